#!/usr/bin/env python
"""bench.py — BASELINE.json headline metric on the C2 workload.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
    (N > 1: either under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py
    --gpus N ...`, or from a bare shell — bench.py then runs itself under torch.distributed.run
    with N ranks on 127.0.0.1, as a child process; rank 0 prints the one JSON line either way)

A plain run sets up, warms up, times the K steps, writes the last step's outputs (--dump-outputs) and
prints the result line.  --full adds what the headline does not need, after the timed steps: the
roofline / per-kernel figures and the box calibration (--no-roofline drops them), the CPU baseline
(--no-cpu-baseline drops it) and, with several ranks, the all-reduce timing.

One "step" = one Clipped-PPO iteration of the hot path on every rank: 2048 env-steps (64 synthetic
Atari-like envs x 32 steps, 84x84x4 uint8 stacked observations) through the vectorised
env-step / filter / store loop, then GAE + 10 epochs x 32 minibatches of 64 (320 gradient updates)
— SURVEY.md §8 config C2, clipped_ppo_agent.py defaults.  value = env-steps/s summed over ranks
(weak scaling: every rank owns its own 64-env vector; the only exchange is the gradient all-reduce).
Inputs are generated on the device (Philox), nothing is staged over PCIe in the timed region.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: what RCCL needs on this pool

import numpy as np  # noqa: E402
import torch  # noqa: E402

N_ENV, EP_LEN, PLAYING_STEPS, BATCH, EPOCHS, N_ACTIONS = 64, 32, 2048, 64, 10, 6
FRAME = (84, 84)
PEAK_FP32_MFMA_TFLOPS = 157.3      # /opt/skills/guides/MI355X_MICROARCH.md, dense fp32 matrix peak


def build_agent(device, dist, seed=0, ep_len=None):
    from coach_amd.agents.clipped_ppo_agent import ClippedPPOAgent, ClippedPPOAgentParameters
    from coach_amd.core_types import EnvironmentSteps
    from coach_amd.environments.synthetic_vector_environment import (
        SyntheticVectorEnvironment, SyntheticVectorEnvironmentParameters)
    ep = SyntheticVectorEnvironmentParameters("image", N_ENV, FRAME, N_ACTIONS, episode_length=ep_len or EP_LEN,
                                              seed=1234)
    env = SyntheticVectorEnvironment(ep, device, rank=dist.rank)
    ap = ClippedPPOAgentParameters()
    ap.seed = seed
    ap.algorithm.num_consecutive_playing_steps = EnvironmentSteps(PLAYING_STEPS)
    ap.algorithm.optimization_epochs = EPOCHS
    ap.network_wrappers["main"].batch_size = BATCH
    return ClippedPPOAgent(ap, env, device, dist=dist)


def one_step(agent):
    res = None
    while res is None:
        agent.act()
        res = agent.train()
    return res


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(out_dir, agent, results):
    """--dump-outputs: what the timed path computed in its last step, as DIR/<name>.npy (float32 / float64) — every
    network's online weights after the step (weights_<network>.npy) and what the step's train() calls returned
    (`results`: name -> device tensor).  An array that would take the files past 64 MB in all is replaced by a fixed,
    seeded sample of its elements (sorted indices, RandomState(0))."""
    arrays = {"weights_%s" % name: net.params.weights for name, net in agent.networks.items()}
    arrays.update(results)
    os.makedirs(out_dir, exist_ok=True)
    total = 0
    for name, t in arrays.items():
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float32)
        if total + a.nbytes > DUMP_LIMIT_BYTES:
            keep = max(0, (DUMP_LIMIT_BYTES - total) // a.itemsize - 1024)
            idx = np.sort(np.random.RandomState(0).choice(a.size, min(keep, a.size), replace=False))
            a = a.reshape(-1)[idx]
        total += a.nbytes
        np.save(os.path.join(out_dir, name + ".npy"), a)


# ------------------------------------------------------------------ the other BASELINE configs
# (parity-test workloads; `--workload c1|c3|c4|c5` times them with the same contract, the default
# and the judged line is c2)
OFF_POLICY = {
    # name: (description, n_env, vector steps per bench step, heat-up vector steps)
    "c1": ("C1: CartPole-like DQN, 1 env, obs 4, 2 actions, uniform replay 40k, B=32, 1 update / env-step", 1, 256, 64),
    "c3": ("C3: Breakout-like DQN + prioritized replay (2^20 transitions, alpha .6, beta .4), 64 envs/GPU, "
           "84x84x4 uint8, B=32, 1 update / 4 env-steps", 64, 64, 64),
    "c4": ("C4: HalfCheetah-like TD3, 256 envs/GPU, obs 17, act 6, twin critic 400-300, B=100, episodes of "
           "100 steps, 1 update / env-step at episode end", 256, 100, 100),
    "c5": ("C5: Humanoid-like SAC, 512 envs/GPU, obs 376, act 17, 256-256 nets, B=256, 1 update / env-step", 512, 8, 4),
}


def build_off_policy(name, device, dist):
    from coach_amd.core_types import EnvironmentSteps
    from coach_amd.environments.synthetic_vector_environment import (
        SyntheticVectorEnvironment, SyntheticVectorEnvironmentParameters as EP)
    from coach_amd.memories.memory import MemoryGranularity
    n_env = OFF_POLICY[name][1]
    if name == "c1":
        from coach_amd.agents.dqn_agent import DQNAgent, DQNAgentParameters
        ap = DQNAgentParameters()
        ap.algorithm.num_consecutive_playing_steps = EnvironmentSteps(1)
        ap.algorithm.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(100)
        ap.network_wrappers["main"].replace_mse_with_huber_loss = False        # presets/CartPole_DQN.py
        ap.memory.max_size = (MemoryGranularity.Transitions, 40000)
        env = SyntheticVectorEnvironment(EP("vector", n_env, (4,), 2, episode_length=200, seed=1234), device, rank=dist.rank)
        return DQNAgent(ap, env, device, dist=dist)
    if name == "c3":
        from coach_amd.agents.dqn_agent import DQNAgent, DQNAgentParameters
        from coach_amd.memories.non_episodic.prioritized_experience_replay import \
            PrioritizedExperienceReplayParameters
        ap = DQNAgentParameters()
        ap.memory = PrioritizedExperienceReplayParameters()
        ap.memory.max_size = (MemoryGranularity.Transitions, 1 << 20)
        from coach_amd.schedules import LinearSchedule
        ap.memory.beta = LinearSchedule(0.4, 1.0, 12500000)                    # presets/Atari_DQN_with_PER.py
        ap.algorithm.reward_clipping = (-1.0, 1.0)
        env = SyntheticVectorEnvironment(EP("image", n_env, FRAME, 4, episode_length=1024, seed=1234), device, rank=dist.rank)
        return DQNAgent(ap, env, device, dist=dist)
    if name == "c4":
        from coach_amd.agents.td3_agent import TD3Agent, TD3AgentParameters
        ap = TD3AgentParameters()
        ap.memory.max_size = (MemoryGranularity.Transitions, 1 << 20)          # 1M rounded to n_env multiples
        env = SyntheticVectorEnvironment(EP("vector", n_env, (17,), None, action_dim=6, episode_length=100, seed=1234),
                                         device, rank=dist.rank)
        return TD3Agent(ap, env, device, dist=dist)
    from coach_amd.agents.soft_actor_critic_agent import SoftActorCriticAgent, SoftActorCriticAgentParameters
    ap = SoftActorCriticAgentParameters()
    ap.memory.max_size = (MemoryGranularity.Transitions, 1 << 20)
    env = SyntheticVectorEnvironment(EP("vector", n_env, (376,), None, action_dim=17, episode_length=1000, seed=1234),
                                     device, rank=dist.rank)
    return SoftActorCriticAgent(ap, env, device, dist=dist)


def _cpu_off_policy_once(name, budget_s=8.0):
    """One timing under the CURRENT BLAS thread setting (see cpu_baseline_off_policy): the oracle's update step (numpy
    restatement of the reference agent's learn_from_batch) and its acting step — ONE forward pass of the acting network
    on ONE state per env-step, which is how the reference acts (one env per process, agent.py:790-830) — each on a
    bounded number of repetitions; env-steps/s = 1 / (acting + updates-per-env-step x update)."""
    import numpy as np
    from coach_amd.nn import graph as G, networks as NW, actor_critic_nets as AC
    rng = np.random.RandomState(0)

    def arrays_of(build):
        params = G.FlatParams()
        mods = build(params)
        params.finalize("cpu")
        r = np.random.RandomState(0)
        for m in mods:
            m.initialize(r)
        return params.named_arrays()

    def timed(fn):
        t0, n = time.perf_counter(), 0
        while n < 2 or (time.perf_counter() - t0 < budget_s and n < 200):
            fn(); n += 1
        return (time.perf_counter() - t0) / n, n

    if name in ("c1", "c3"):
        from oracle.agents import DQNOracle
        shape, A, B = ((4,), 2, 32) if name == "c1" else (FRAME + (4,), 4, 32)

        def build(p):
            torso, feat = NW.build_torso(p, "main", shape, "relu", 1)
            return [torso, G.Dense(p, "main/q_head/dense", feat, A, None, 1)]
        o = DQNOracle(arrays_of(build), shape, A, huber=(name == "c3"))
        obs = rng.randint(0, 256, size=(B,) + shape).astype(np.uint8) if name == "c3" else rng.randn(B, 4).astype(np.float32)
        a, r, d = rng.randint(0, A, B), rng.randn(B).astype(np.float32), rng.rand(B) < 0.1
        t, n = timed(lambda: o.learn_from_batch(obs, obs, a, r, d, 0.99))
        ta, na = timed(lambda: o.q(obs[:1]))
        per_step = 1.0 if name == "c1" else 0.25
    elif name == "c4":
        from oracle import ac_nets as O
        D, A, B = 17, 6, 100

        def ba(p):
            e, f = AC._mlp(p, "actor/embedder", D, (400,), "relu"); m, f = AC._mlp(p, "actor/middleware", f, (300,), "relu")
            return [e, m, G.Dense(p, "actor/ddpg_actor_head/fc_mean", f, A, "tanh")]

        def bc(p):
            m, f = AC._mlp(p, "critic/middleware", D + A, (400, 300), "relu", towers=2)
            return [m, G.Dense(p, "critic/v_head/output", f, 1, None, 2)]
        oa, oc = O.ActorOracle(arrays_of(ba), 1.0, lr=1e-3), O.CriticOracle(arrays_of(bc), streams=2)
        batch = (rng.randn(B, D).astype(np.float32), rng.uniform(-1, 1, (B, A)).astype(np.float32),
                 rng.randn(B).astype(np.float32), np.zeros(B, bool), rng.randn(B, D).astype(np.float32))
        it = [0]

        def f():
            it[0] += 1
            O.td3_update(oa, oc, batch, rng.normal(0, 0.2, (B, A)), it[0], -np.ones(A, np.float32), np.ones(A, np.float32))
        t, n = timed(f)
        ta, na = timed(lambda: oa.forward(batch[0][:1]))
        per_step = 1.0
    else:
        from oracle import ac_nets as O
        D, A, B = 376, 17, 256

        def mlp2(prefix, head, n_out):
            def b(p):
                e, f = AC._mlp(p, prefix + "/embedder", D, (256,), "relu"); m, f = AC._mlp(p, prefix + "/middleware", f, (256,), "relu")
                return [e, m, G.Dense(p, head, f, n_out, None)]
            return b

        def bq(p):
            return [G.Dense(p, "q/q_head/obs_fc", D, 256, "relu", 2), G.Dense(p, "q/q_head/act_fc", A, 256, "relu", 2),
                    G.Dense(p, "q/q_head/fc1", 256, 256, "relu", 2), G.Dense(p, "q/q_head/q_output", 256, 1, None, 2)]
        op = O.SACPolicyOracle(arrays_of(mlp2("policy", "policy/sac_policy_head/policy_mu_logsig", 2 * A)))
        ov = O.SACValueOracle(arrays_of(mlp2("v", "v/v_values_head/output", 1)))
        oq = O.SACQOracle(arrays_of(bq))
        batch = (rng.randn(B, D).astype(np.float32), rng.uniform(-1, 1, (B, A)).astype(np.float32),
                 rng.randn(B).astype(np.float32), np.zeros(B, bool), rng.randn(B, D).astype(np.float32))
        t, n = timed(lambda: O.sac_update(op, oq, ov, batch, rng.standard_normal((3, B, A))))
        ta, na = timed(lambda: op.forward(batch[0][:1], rng.standard_normal((1, A))))
        per_step = 1.0
    step_s = ta + t * per_step
    return {"value": round(1.0 / step_s, 2), "unit": "env-steps/s", "grad_updates_per_s": round(per_step / step_s, 2),
            "update_s": t, "act_s": ta,
            "sample": "%d update steps at %.4f s + %d acting forward passes (one state each) at %.5f s; %.2f updates per "
                      "env-step" % (n, t, na, ta, per_step)}


def cpu_baseline_off_policy(name, budget_s=12.0):
    """`cpu_baseline` of the off-policy workloads, like C2's (cpu_baseline below): the oracle timed under three BLAS
    thread settings on this box — ONE thread, the reference's own setting (coach.py:666 OMP_NUM_THREADS=1;
    graph_manager.py:219-220 intra / inter-op 1) and the figure reported as `value`; 8 threads; every host core —
    acting cost included."""
    try:
        from threadpoolctl import threadpool_info, threadpool_limits
        all_cores = max([p_.get("num_threads", 1) for p_ in threadpool_info()] + [1])
    except Exception:
        threadpool_limits, all_cores = None, os.cpu_count() or 1
    settings = [1] if threadpool_limits is None else sorted({1, min(8, all_cores), all_cores})
    runs = {}
    for th in settings:
        if threadpool_limits is None:
            runs[th] = _cpu_off_policy_once(name, budget_s)
        else:
            with threadpool_limits(limits=th):
                runs[th] = _cpu_off_policy_once(name, budget_s / len(settings))
    one = runs[settings[0]]
    return {"value": one["value"], "unit": "env-steps/s", "cores": settings[0], "kind": "port",
            "grad_updates_per_s": one["grad_updates_per_s"], "host_cores": os.cpu_count(),
            "sample": "oracle/ (numpy fp32 restatement of rl_coach's CPU path), %d BLAS thread(s) — the reference runs "
                      "single-threaded: %s" % (settings[0], one["sample"]),
            "by_threads": {str(th): {"value": r["value"], "grad_updates_per_s": r["grad_updates_per_s"], "cores": th,
                                     "update_s": round(r["update_s"], 5), "act_s": round(r["act_s"], 6)}
                           for th, r in runs.items()}}




def prefill_c3(agent):
    """the C3 replay is PRE-FILLED — 2^20 transitions, priorities |N(0,1)| + 1e-6 — before
    anything is timed, so that the sampled payload gather walks 7.4 GB of frames instead of a
    cache-resident corner of the ring.  The rows come from real env steps (fixed action, no host draws:
    np.random is left untouched), the priorities from one rlx_per_update per 1024 leaves."""
    from coach_amd.core_types import RunPhase
    mem = agent.memory
    cap = mem.power_of_2_size
    agent.phase = RunPhase.HEATUP
    agent.actions.zero_()
    saved = agent.random_actions
    agent.random_actions = lambda: agent.actions
    try:
        for _ in range(cap // agent.n_env + 1):          # + 1: the last step's rows become visible
            agent.act()
    finally:
        agent.random_actions = saved
    assert mem.count == cap and mem.num_transitions() == cap
    g = torch.Generator(device="cpu").manual_seed(0)
    err = torch.randn(cap, generator=g, dtype=torch.float64).abs().to(agent.device)
    idx = torch.arange(cap, dtype=torch.int32, device=agent.device)
    for i in range(0, cap, 1024):
        mem.update_priorities(idx[i:i + 1024], err[i:i + 1024])    # p = |N(0,1)| + epsilon (1e-6)
    mem.check_status()
    torch.cuda.synchronize()


# algorithmic flops of one update as the REFERENCE executes it (2 * MACs, forward + backward = 3x
# forward, every pass the reference runs), and the dominant kernel family of each workload
UPDATE_FLOPS = {"c1": 43e6, "c3": 3.0e9, "c4": 0.34e9, "c5": 2.3e9}
LAUNCH_FLOOR_US = 1.7      # a dependent trivial kernel inside a hipGraph on MI355X (profiles/r02_launch_cost_microbench.txt)


def update_roofline(agent, workload, reps=200):
    """The off-policy workloads are LATENCY-bound: one update is a chain of dependent small launches.
    Reported: the update's duration measured live with device events over `reps` back-to-back replays of the captured
    update on one sampled batch, the library calls one eager update makes, and what that implies —
    achieved = algorithmic flops / measured duration against the fp32 MFMA peak, and the floor launches x 1.7 us."""
    from coach_amd import _rlx
    B = agent.batch_size
    batch = agent.memory.sample(B)
    saved = agent.use_graphs
    agent.use_graphs = False
    c0 = _rlx.CALL_COUNT
    agent.learn_from_batch(batch)
    calls = _rlx.CALL_COUNT - c0
    agent.use_graphs = saved
    # The update's host draws (TD3: the smoothing noise, SAC: three normal draws of B x A — ~100-200 us of np.random per
    # update, more than the device needs for the update itself) are made ONCE and staged, as the training loop stages them
    # with the sampled rows: what is timed is the device's duration of the captured update, not the host's RNG.
    host_draw_us = None
    fields = getattr(agent, "_update_record_fields", lambda: None)()
    if fields:
        import time as _time
        t0 = _time.perf_counter()
        for _ in range(20):
            draw = agent._draw_update_host()
        host_draw_us = 1e6 * (_time.perf_counter() - t0) / 20
        agent._staged = {k: torch.as_tensor(v, device=agent.device) for k, v in draw.items()}
    try:
        for _ in range(3):
            agent.learn_from_batch(batch)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            agent.learn_from_batch(batch)
        e1.record()
        e1.synchronize()
    finally:
        agent._staged = None
    us = 1e3 * e0.elapsed_time(e1) / reps
    flops = UPDATE_FLOPS[workload]
    achieved = flops / (us * 1e-6) / 1e12
    return {"bound": "mfma", "achieved": round(achieved, 3), "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
            "frac": round(achieved / PEAK_FP32_MFMA_TFLOPS, 5), "traffic": None,
            "kernel": "one gradient update (learn_from_batch: forward passes, targets, loss, backward, Adam) as captured",
            "update_us": round(us, 2), "update_flops": flops, "library_calls_per_update": calls,
            "host_draws_us_per_update": None if host_draw_us is None else round(host_draw_us, 1),
            "latency_model": {"launch_floor_us": LAUNCH_FLOOR_US, "floor_us": round(calls * LAUNCH_FLOOR_US, 1),
                              "note": "latency-bound: the floor of `calls` dependent launches, not the MFMA rate, "
                                      "bounds this update (a call may launch 1-2 kernels)"}}


def run_off_policy(args, device, dist):
    from coach_amd.core_types import RunPhase
    desc, n_env, vsteps, heat = OFF_POLICY[args.workload]
    agent = build_off_policy(args.workload, device, dist)
    if args.workload == "c3" and not args.no_prefill:
        prefill_c3(agent)
        desc += "; replay pre-filled with 2^20 transitions, priorities |N(0,1)|+1e-6"
    agent.phase = RunPhase.HEATUP
    for _ in range(heat):
        agent.act()
    agent.phase = RunPhase.TRAIN

    fused_step = getattr(agent, "step_and_train", None)      # act() + train() as one record + one graph replay
    last_loss = [None]                                       # the loss train() returned last (--dump-outputs)

    def step():
        for _ in range(vsteps):
            if fused_step is not None:
                loss = fused_step()
            else:
                agent.act()
                loss = agent.train()
            if loss is not None:
                last_loss[0] = loss
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
    sampler = LoadSampler() if dist.rank == 0 and args.full and not args.no_roofline else None
    it0, t0 = agent.training_iteration, time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize(); dist.barrier(); torch.cuda.synchronize()
    elapsed = dist.max_over_ranks(time.perf_counter() - t0)
    agent.check_status()
    if args.dump_outputs and dist.rank == 0:
        dump_outputs(args.dump_outputs, agent, {} if last_loss[0] is None else {"last_loss": last_loss[0]})
    updates = dist.sum_over_ranks(agent.training_iteration - it0)
    env_steps = dist.world_size * n_env * vsteps * args.steps
    out = {"metric": "env-steps/sec (+ grad-updates/sec), %s" % args.workload.upper(),
           "value": round(env_steps / elapsed, 1), "unit": "env-steps/s", "n_gpus": dist.world_size,
           "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
           "grad_updates_per_s": round(updates / elapsed, 1),
           "config": {"workload": desc, "env_steps_per_step_per_gpu": n_env * vsteps,
                      "parallelism": "dp%d" % dist.world_size, "hip_graphs": bool(agent.use_graphs)},
           "episode_stats": {k: (v if np.isfinite(v) else None) for k, v in agent.episode_statistics().items()}}
    if dist.rank == 0 and args.full and not args.no_roofline and dist.world_size == 1:
        out["roofline"] = update_roofline(agent, args.workload)
        out["box"] = box_calibration(device)
        out["box"]["under_load"] = sampler.result() if sampler else None
    if dist.rank == 0 and dist.world_size == 1 and args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline_off_policy(args.workload)
        # the reference's own per-step / per-update code, timed in the build container (tools/time_reference_cpu*.py)
        ref_file = {"c1": "r01_cpu_reference_c1_container.json"}.get(
            args.workload, "r02_cpu_reference_%s_container.json" % args.workload)
        try:
            with open(os.path.join(ROOT, "profiles", ref_file)) as f:
                r = json.load(f)
            out["cpu_baseline"]["reference"] = {k: r[k] for k in ("value", "unit", "cores", "kind", "where", "sample")}
        except (OSError, ValueError, KeyError):
            pass
    finish(dist, out)


# ------------------------------------------------------------------------------------- roofline
GEMM_FAMILY = ("gemm_", "splitk_reduce", "conv23_", "conv32_", "conv_dw_", "ppo_fc_heads")   # kernels that issue (or finish) fp32 MFMA products


def _family(name):
    if name.startswith(GEMM_FAMILY):
        return "gemm"
    for key, fam in (("col2im", "col2im"), ("conv_", "col2im"), ("ppo_", "heads"), ("dense_small", "heads"),
                     ("adam", "adam"), ("img_gather", "gather"), ("copy_columns", "gather")):
        if name.startswith(key):
            return fam
    return "other"


def in_update_kernel_trace(agent, n_updates=16, warm=4):
    """IN-UPDATE kernel durations: `n_updates` consecutive eager minibatch updates on the epoch buffers of the last
    training phase, every kernel timed by its own dispatch timestamps (librlx's in-process timer, rlx_profile_* —
    what `rocprofv3 --kernel-trace` reports per dispatch).  Operands are as the previous kernel of the update left
    them; this is the figure `roofline.frac` is built on.  Returns (per-update microseconds by kernel name, by
    family, launches per update)."""
    from coach_amd import _rlx
    saved_graphs, saved_steps = agent.use_graphs, agent.memory.steps
    agent.use_graphs = False
    agent.memory.steps = agent.steps_per_phase      # the (cleaned) rollout's rows are still in HBM
    try:
        epoch = agent._gather_epoch(PLAYING_STEPS)
        for i in range(warm):
            agent._minibatch_fb(BATCH, None, i=i, epoch=epoch)
            agent._minibatch_finish(1.0)
        torch.cuda.synchronize()
        with _rlx.KernelTimer(256 * n_updates) as timer:
            for i in range(n_updates):
                agent._minibatch_fb(BATCH, None, i=(warm + i) % (PLAYING_STEPS // BATCH), epoch=epoch)
                agent._minibatch_finish(1.0)
            torch.cuda.synchronize()
    finally:
        agent.use_graphs, agent.memory.steps = saved_graphs, saved_steps
    by_name, by_family, calls = {}, {}, {}
    for name, us in timer.records:
        by_name[name] = by_name.get(name, 0.0) + us / n_updates
        calls[name] = calls.get(name, 0) + 1
        fam = _family(name)
        by_family[fam] = by_family.get(fam, 0.0) + us / n_updates
    table = [{"kernel": k, "launches_per_update": calls[k] / n_updates, "us_per_update": round(v, 2),
              "avg_us": round(v * n_updates / calls[k], 2)} for k, v in sorted(by_name.items(), key=lambda kv: -kv[1])]
    return table, {k: round(v, 2) for k, v in by_family.items()}, len(timer.records) / n_updates


def epoch_graph_update_us(agent, reps=5):
    """one minibatch update inside the captured epoch graph (what the timed region replays): device events around
    `reps` replays of the epoch graph / minibatches per epoch (the epoch's gather launches included)."""
    graphs = [g for k, g in agent._graphs.items() if k and k[0] == "epoch"]
    if not graphs:
        return None
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    graphs[0].replay()
    e0.record()
    for _ in range(reps):
        graphs[0].replay()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps / (PLAYING_STEPS // BATCH)


class LoadSampler(object):
    """clock / power / busy readings of the card this process computes on, and of the host's OTHER cards (other tenants),
    taken by a separate process (tools/box_info.py --sample) WHILE the timed region runs: `box.under_load`."""

    def __init__(self, seconds=3.0):
        import subprocess
        try:
            self.p = subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "box_info.py"), "--sample", str(seconds)],
                                      stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        except Exception:
            self.p = None

    def result(self):
        if self.p is None:
            return None
        try:
            out, _ = self.p.communicate(timeout=20)
            return json.loads(out.strip().splitlines()[-1])
        except Exception:
            return None


def box_settings():
    """what kind of box this is (driver / firmware / module parameters / partition modes / which card of the host / what the
    neighbours are doing): tools/box_info.py summary()."""
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import box_info
        return box_info.summary()
    except Exception as e:
        return {"error": str(e)[:200]}


def box_calibration(device):
    """A two-second fixed calibration of THIS box, so that bench lines from different boxes of the pool can be compared
    (the pool's boxes differ by up to 30 % on identical code): device-to-device copy rate, a compute-bound 4096^3 fp32
    MFMA product, and the cost of one dependent trivial launch inside a hipGraph."""
    from coach_amd import _rlx
    out = {}
    try:
        out["device"] = torch.cuda.get_device_name(device)
        out["compute_units"] = torch.cuda.get_device_properties(device).multi_processor_count
    except Exception:
        pass
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 64 << 20
    a, b = torch.empty(n, dtype=torch.uint8, device=device), torch.zeros(n, dtype=torch.uint8, device=device)
    for _ in range(3):
        a.copy_(b)
    e0.record()
    for _ in range(20):
        a.copy_(b)
    e1.record(); e1.synchronize()
    out["copy_64MiB_GBps"] = round(2 * n * 20 / (e0.elapsed_time(e1) * 1e-3) / 1e9, 1)     # read + write
    M = 4096
    A = torch.randn(M, M, device=device)
    B = torch.randn(M, M, device=device)
    C = torch.empty(M, M, device=device)
    for _ in range(2):
        _rlx.gemm(M, M, M, A, B, C)
    e0.record()
    for _ in range(5):
        _rlx.gemm(M, M, M, A, B, C)
    e1.record(); e1.synchronize()
    out["gemm_4096_fp32_TFLOPs"] = round(2.0 * M ** 3 * 5 / (e0.elapsed_time(e1) * 1e-3) / 1e12, 1)
    # beyond the 256 MiB Infinity Cache: 1 GiB device-to-device (HBM rate), and the latency of a dependent load — a
    # pointer chase over 512 MiB (HBM) and over 16 MiB (what the Infinity Cache / L2 answer) in 256-byte strides.  These
    # are what separates the pool's box classes (the 64 MiB copy and the MFMA rate above do not).
    try:
        big = torch.empty(1 << 30, dtype=torch.uint8, device=device)
        big2 = torch.empty(1 << 30, dtype=torch.uint8, device=device)
        big2.copy_(big)
        e0.record()
        for _ in range(4):
            big2.copy_(big)
        e1.record(); e1.synchronize()
        out["copy_1GiB_GBps"] = round(2 * (1 << 30) * 4 / (e0.elapsed_time(e1) * 1e-3) / 1e9, 1)
        del big2
        lib = _rlx.lib()
        res = torch.zeros(1, dtype=torch.int32, device=device)
        for name, nodes in (("chase_512MiB_ns", 1 << 21), ("chase_16MiB_ns", 1 << 16)):
            perm = torch.randperm(nodes, device=device, generator=torch.Generator(device=device).manual_seed(1)).int()
            chain = big[:nodes * 256].view(torch.int32)                       # one used word per 256 bytes
            chain[perm.long() * 64] = torch.roll(perm, -1) * 64
            steps = 4096
            lib.probe_chase(chain, int(perm[0].item()) * 64, 256, res, _rlx.current_stream())
            e0.record()
            lib.probe_chase(chain, int(perm[0].item()) * 64, steps, res, _rlx.current_stream())
            e1.record(); e1.synchronize()
            out[name] = round(1e6 * e0.elapsed_time(e1) / steps, 1)
        del big
    except Exception as e:                                                  # (a box short of memory: skip, say so)
        out["memory_probe_error"] = str(e)[:120]
    # the matrix pipe itself: cycles per dependent fp32 32x32x2 MFMA and the clock the shader holds with every CU busy on
    # them (rlx_probe_mfma) — the denominator of roofline.frac assumes 64 cycles at 2.4 GHz
    try:
        wgs, iters = 1024, 8192
        probe = torch.zeros(2 * wgs, dtype=torch.int64, device=device)
        sink = torch.zeros(1, dtype=torch.float32, device=device)
        for _ in range(2):
            _rlx.lib().probe_mfma(wgs, iters, probe, sink, _rlx.current_stream())
        torch.cuda.synchronize()
        pr = probe.cpu().numpy().reshape(wgs, 2).astype(np.float64)
        out["shader_MHz_under_mfma"] = int(round(float(np.median(pr[:, 0] / pr[:, 1])) * 100.0))
    except Exception as e:
        out["mfma_probe_error"] = str(e)[:120]
    # issue rate vs dependent latency of the two fp32 MFMA shapes (rlx_probe_mfma_shape; guide: 64 / 64 and 32 / 40 cycles)
    try:
        wgs, iters, cyc = 256, 8192, {}
        probe = torch.zeros(2 * wgs, dtype=torch.int64, device=device)
        sink = torch.zeros(1, dtype=torch.float32, device=device)
        for small, chains in ((0, 1), (0, 2), (1, 1), (1, 2)):
            for _ in range(2):
                _rlx.lib().probe_mfma_shape(wgs, iters, small, chains, probe, sink, _rlx.current_stream())
            torch.cuda.synchronize()
            pr = probe.cpu().numpy().reshape(wgs, 2).astype(np.float64)
            cyc["%s_%dchain" % ("16x16x4" if small else "32x32x2", chains)] = round(float(np.median(pr[:, 0])) / (iters * chains), 1)
        out["mfma_cycles_per_instruction"] = cyc
    except Exception as e:
        out["mfma_shape_probe_error"] = str(e)[:120]
    x = torch.zeros(4, dtype=torch.float32, device=device)
    x.add_(0.0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(500):
            x.add_(0.0)
    g.replay()
    e0.record()
    for _ in range(4):
        g.replay()
    e1.record(); e1.synchronize()
    out["graph_dependent_launch_us"] = round(1e3 * e0.elapsed_time(e1) / (4 * 500), 2)
    del a, b, A, B, C
    out["settings"] = box_settings()
    return out


def gemm_roofline(agent, reps=20):
    """Per-launch timing of the dominant kernel family (gemm_kernel<...>, fp32 MFMA) with HIP events
    on the launch stream: every GEMM descriptor issued by one minibatch update is recorded, then
    each is launched `reps` times back to back between one event pair."""
    import ctypes
    from coach_amd import _rlx
    lib = _rlx.lib()
    recorded = []
    saved_graphs = agent.use_graphs
    agent.use_graphs = False
    _rlx.GEMM_HOOK = recorded.append
    saved_steps = agent.memory.steps
    agent.memory.steps = agent.steps_per_phase      # the (cleaned) rollout's rows are still in HBM
    try:
        # one eager minibatch update on the buffers left over from the last training phase
        agent._minibatch_fb(BATCH, 1.0)
        agent._minibatch_finish(1.0)
    finally:
        _rlx.GEMM_HOOK = None
        agent.use_graphs = saved_graphs
        agent.memory.steps = saved_steps
    torch.cuda.synchronize()
    stream = _rlx.current_stream()
    ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
    lib.event_create(ctypes.byref(ev0))
    lib.event_create(ctypes.byref(ev1))
    total_ms, total_flops, per_shape = 0.0, 0.0, []
    n_products = 0
    for rec in recorded:
        # one record = ONE library call of the GEMM family exactly as the update issued it (a layer's dW + dX pair, a
        # direct convolution input gradient, the deferred split-K reductions of a backward pass ...): the products it
        # stands for and a thunk that issues it again
        descs, run = rec["descs"], rec["run"]
        for _ in range(3):
            run()
        lib.event_record(ev0, stream)
        for _ in range(reps):
            run()
        lib.event_record(ev1, stream)
        ms = ctypes.c_float()
        lib.event_elapsed_ms(ev0, ev1, ctypes.byref(ms))
        flops = rec["flops"] if rec["flops"] is not None else sum(2.0 * x.M * x.N * x.K * x.batch for x in descs)
        total_ms += ms.value / reps
        total_flops += flops
        n_products += len(descs)
        per_shape.append({"products": [{"M": x.M, "N": x.N, "K": x.K, "batch": x.batch} for x in descs],
                          "us": 1e3 * ms.value / reps, "tflops": flops / (ms.value / reps * 1e-3) / 1e12})
    lib.event_destroy(ev0)
    lib.event_destroy(ev1)
    n = len(recorded)
    warm_tflops = total_flops / (total_ms * 1e-3) / 1e12
    # algorithmic bytes of the products as GEMMs (A as addressed — the im2col-expanded volume for the convolutions —
    # + B + C), from the recorded descriptors
    operand_bytes = sum((x.M * x.K * (1 if x.a_is_u8 else 4) + x.K * x.N * 4 + x.M * x.N * 4) * x.batch
                        for rec in recorded for x in rec["descs"])
    # ---- the headline: the same family timed IN the update (see in_update_kernel_trace)
    table, fam, launches = in_update_kernel_trace(agent)
    gemm_us = fam.get("gemm", 0.0)
    achieved = total_flops / (gemm_us * 1e-6) / 1e12
    update_us = epoch_graph_update_us(agent)
    # HBM-side bytes of the GEMM family per launch: PMC passes cannot run inside this process, so the figure is the
    # committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE measurement of the same update (tools/ppo_update_once.py +
    # tools/pmc_summary.py -> profiles/r0N_pmc_gemm_traffic.json; the x 2 on FETCH_SIZE is calibrated on this library's
    # own loads, profiles/r03_pmc_calibration.json); used only if that file describes the same products AND launches.
    gemm_launches = sum(r["launches_per_update"] for r in table if r["kernel"].startswith(GEMM_FAMILY))
    traffic = None
    for fn in ("r06_pmc_gemm_traffic.json", "r05_pmc_gemm_traffic.json", "r04_pmc_gemm_traffic.json", "r03_pmc_gemm_traffic.json"):
        try:
            with open(os.path.join(ROOT, "profiles", fn)) as f:
                pm = json.load(f)
            if pm.get("gemm_products") == n_products and \
                    pm.get("gemm_launches", 0) + pm.get("reduce_launches", 0) == round(gemm_launches):
                traffic = round(pm["traffic_bytes_per_update"] / n)
                break
        except (OSError, ValueError, KeyError):
            pass
    return {"bound": "mfma", "achieved": round(achieved, 3), "peak": PEAK_FP32_MFMA_TFLOPS,
            "unit": "TFLOP/s", "frac": round(achieved / PEAK_FP32_MFMA_TFLOPS, 4), "traffic": traffic,
            "timing": "IN-UPDATE: per-dispatch begin/end timestamps (librlx rlx_profile_*, = rocprofv3 --kernel-trace "
                      "durations) of every GEMM-family kernel over 16 consecutive eager minibatch updates, summed per update",
            "gemm_us_per_update": round(gemm_us, 1), "gemm_launches_per_update": round(gemm_launches, 2),
            "frac_warm": round(warm_tflops / PEAK_FP32_MFMA_TFLOPS, 4),
            "gemm_us_per_update_warm": round(1e3 * total_ms, 1),
            "warm_timing": "each library call of the family replayed %d x back to back between one event pair" % reps,
            "traffic_unit": "bytes per library call of the GEMM family, split-K reduces included (2 x FETCH_SIZE + WRITE_SIZE, "
                            "PMC passes of tools/ppo_update_once.py); operands (A as addressed) and results of the %d "
                            "products are %.1fe6 bytes per call" % (n_products, operand_bytes / 1e6 / n),
            "kernel": "gemm_dma_kernel / gemm_dma_pair_kernel (LDS-DMA ring), gemm_fast_kernel (uint8 frames), "
                      "conv23_forward_kernel (conv1 -> conv2 -> conv3 forward per half image, activations in LDS) + split-K reduces "
                      "(fp32 MFMA 32x32x2): %d products in %d library calls per minibatch update" % (n_products, n),
            "limiter": "measured (profiles/r04_slab_step_ablation.txt, profiles/r05_ab_*.txt): the tiled launches are bound by "
                       "operand delivery — fills in flight from beyond the XCD's L2, every kernel of the update starts cold — "
                       "with the MFMA chain hidden under it; co-resident independent work does not overlap (it lengthens the "
                       "fills), only fewer bytes through the CUs help: conv23_forward_kernel keeps conv1's and conv2's output in LDS "
                       "and runs at 0.45 MFMA-busy; the MFMA peak stays the denominator of frac",
            "flops_per_update": total_flops, "flops_per_launch": total_flops / n,
            "avg_launch_us": round(gemm_us / max(gemm_launches, 1), 2),
            "update_us_by_family": fam, "kernel_launches_per_update": round(launches, 1),
            "update_us_sum_of_kernels": round(sum(fam.values()), 1),
            "update_us_in_epoch_graph": None if update_us is None else round(update_us, 1),
            "update_kernels": table}, per_shape


# ---------------------------------------------------------------------------------- cpu baseline
def _cpu_baseline_once(budget_s):
    """One timing of the oracle's C2 iteration under the CURRENT BLAS thread setting (see cpu_baseline)."""
    import random
    from oracle.agents import ClippedPPOAgentOracle
    from oracle.synth_env import SynthVecEnv
    from coach_amd.nn import graph as G, networks as NW
    # same topology / init as the HIP net, built on the host without touching the GPU library
    params = G.FlatParams()
    torso, feat = NW.build_torso(params, "main", FRAME + (4,), "tanh", 2)
    vh = G.Dense(params, "main/v_head/dense", feat, 1, None, 1, init=G.normalized_columns(1.0))
    ph = G.Dense(params, "main/ppo_head/policy_fc", feat, N_ACTIONS, None, 1)
    params.finalize("cpu")
    rng = np.random.RandomState(0)
    for m in (torso, vh, ph):
        m.initialize(rng)
    arrays = params.named_arrays()
    env = SynthVecEnv(0, N_ENV, FRAME[0] * FRAME[1], EP_LEN, 1234)
    o = ClippedPPOAgentOracle(arrays, env, N_ACTIONS, batch_size=BATCH, playing_steps=PLAYING_STEPS,
                              epochs=EPOCHS)
    random.seed(0)
    np.random.seed(0)
    o.reset(FRAME)
    t0 = time.perf_counter()
    n_act = 0
    while n_act < 2 or (time.perf_counter() - t0 < 0.2 * budget_s and n_act < 8):
        o.act()
        n_act += 1
    t_act = (time.perf_counter() - t0) / n_act
    states = np.stack(o.cur)
    t0 = time.perf_counter()
    o.net.values(states)
    t_val = time.perf_counter() - t0
    frozen = o.net.clone_policy()
    acts = np.random.randint(0, N_ACTIONS, size=BATCH)
    adv = np.random.randn(BATCH).astype(np.float32)
    vt = np.random.randn(BATCH).astype(np.float32)
    t0 = time.perf_counter()
    n_mb = 0
    while n_mb < 2 or (time.perf_counter() - t0 < 0.6 * budget_s and n_mb < 12):
        old = o.net.policy_probs(states, frozen)
        o.net.train_minibatch(states, acts, adv, vt, old)
        n_mb += 1
    t_mb = (time.perf_counter() - t0) / n_mb
    n_updates = EPOCHS * (PLAYING_STEPS // BATCH)
    t_iter = EP_LEN * t_act + (PLAYING_STEPS // BATCH) * t_val + n_updates * t_mb
    return {"value": round(PLAYING_STEPS / t_iter, 2), "unit": "env-steps/s",
            "grad_updates_per_s": round(n_updates / t_iter, 3),
            "sample": "%d vector env-steps (64 envs), 1 value chunk and %d minibatch updates timed, scaled to one full "
                      "iteration (32 steps + 32 value chunks + 320 updates); %.3f s/step, %.3f s/chunk, %.3f s/update"
                      % (n_act, n_mb, t_act, t_val, t_mb)}


def cpu_baseline(budget_s=24.0):
    """The oracle (numpy fp32 restatement of the reference's CPU path) on a bounded sample of the same workload: a few
    vector env-steps, value chunks and minibatch updates are timed and scaled to one full iteration (32 steps, 32
    value chunks of 64, 320 updates incl. the per-minibatch old-policy pass the reference performs).  Timed under
    three BLAS thread settings: ONE thread — the reference's own setting (coach.py:666 OMP_NUM_THREADS=1, TF
    intra/inter-op 1, graph_manager.py:219-220) and the figure reported as `value` — 8 threads, and every host core."""
    try:
        from threadpoolctl import threadpool_info, threadpool_limits
        all_cores = max([p.get("num_threads", 1) for p in threadpool_info()] + [1])
    except Exception:
        threadpool_limits, all_cores = None, os.cpu_count() or 1
    settings = [1] if threadpool_limits is None else sorted({1, min(8, all_cores), all_cores})
    runs = {}
    for th in settings:
        if threadpool_limits is None:
            runs[th] = _cpu_baseline_once(budget_s)
        else:
            with threadpool_limits(limits=th):
                runs[th] = _cpu_baseline_once(budget_s / len(settings))
    one = runs[settings[0]]
    out = {"value": one["value"], "unit": "env-steps/s", "cores": settings[0], "kind": "port",
           "sample": "oracle/ (numpy fp32 restatement of rl_coach's CPU path), %d BLAS thread(s) — the reference runs "
                     "single-threaded: %s" % (settings[0], one["sample"]),
           "grad_updates_per_s": one["grad_updates_per_s"], "host_cores": os.cpu_count(),
           "by_threads": {str(th): {"value": r["value"], "grad_updates_per_s": r["grad_updates_per_s"], "cores": th}
                          for th, r in runs.items()}}
    return out


def dry_run(args):
    """The multi-rank contract without the hot path: rendezvous (gloo), K timed no-op steps bracketed by
    barriers, max-over-ranks time, whole-job sum, ONE JSON line from rank 0."""
    from coach_amd.distributed import GradientSync
    dist = GradientSync(backend="gloo")
    if dist.world_size != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, dist.world_size))
    flat = torch.ones(1024)
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        if dist.enabled:
            dist.all_reduce_sum(flat)
            flat /= dist.world_size
    dist.barrier()
    elapsed = dist.max_over_ranks(time.perf_counter() - t0)
    units = dist.sum_over_ranks(args.steps)
    if dist.rank == 0:
        print(json.dumps({"metric": "dry-run steps/s", "value": round(units / max(elapsed, 1e-9), 1), "unit": "steps/s",
                          "n_gpus": dist.world_size, "steps": args.steps, "warmup": args.warmup,
                          "ms_per_step": round(1e3 * elapsed / max(args.steps, 1), 3), "higher_is_better": True,
                          "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "none",
                          "config": {"workload": "dry run (no kernels)", "parallelism": "dp%d" % dist.world_size},
                          "allreduce_check": float(flat[0])}))
    dist.barrier()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--force-dist", action="store_true",
                    help="take the collective path (RCCL) even with one rank: its structural cost at world size 1")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--full", action="store_true",
                    help="after the headline line's timed steps, also measure what it does not need: the roofline / "
                         "per-kernel figures, the box calibration and load sampler, the CPU baseline, the all-reduce timing")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the timed path computed in its last step to DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline and box figures")
    ap.add_argument("--shapes", action="store_true", help="print the per-GEMM-shape table to stderr")
    ap.add_argument("--workload", default="c2", choices=["c1", "c2", "c3", "c4", "c5"],
                    help="BASELINE.json config (default c2 = the headline metric's configuration)")
    ap.add_argument("--no-prefill", action="store_true", help="c3: skip the 2^20-transition pre-fill")
    ap.add_argument("--sac-branches", type=int, default=None, choices=[0, 1],
                    help="A/B (c5): the SAC update's policy / V / Q passes as parallel branches of the captured graph (1, "
                         "the default) or in sequence (0)")
    ap.add_argument("--gemm-pipeline", type=int, default=None, choices=[0, 1],
                    help="A/B: main loop of the fast tiled GEMM kernels (rlx_gemm_pipeline): 1 = LDS-DMA ring (the "
                         "library's default), 0 = register-staged")
    ap.add_argument("--direct-conv-dx", default=None, choices=["0", "1", "always"],
                    help="A/B: convolution input gradients as one windowed-gather product (nn.graph.DIRECT_CONV_INPUT_GRAD)")
    ap.add_argument("--big-tiles", type=int, default=None, choices=[0, 1],
                    help="A/B: several accumulator tiles per wave for large products (rlx_gemm_big_tiles; 1 = default)")
    ap.add_argument("--multi-dw", type=int, default=None, choices=[0, 1],
                    help="A/B: the convolution layers' weight gradients as one launch behind the dX chain (nn.graph.MULTI_DW)")
    ap.add_argument("--conv23-depth", type=int, default=None, help="A/B: weight slabs in rlx_conv23_forward's ring")
    ap.add_argument("--conv23-step", type=int, default=2, help="A/B: slabs per synchronisation step of rlx_conv23_forward")
    ap.add_argument("--fuse-conv", type=int, default=None, choices=[0, 1, 2],
                    help="A/B: the torso's forward convolutions as one launch — 0: three tiled launches, 1: conv2 -> conv3 fused "
                         "(nn.graph.FUSE_CONV_PAIR), 2 = the default: conv1 in front of them too (FUSE_CONV_FIRST)")
    ap.add_argument("--fuse-acting", type=int, default=None, choices=[0, 1],
                    help="A/B (c2): an acting step's small launches merged (ClippedPPOAgent.FUSE_ACTING_LAUNCHES; 1 = default)")
    ap.add_argument("--record-acting", type=int, default=None, choices=[0, 1],
                    help="A/B (c2): the acting steps leave V(s) and the action probabilities in the rollout — no whole-dataset "
                         "value / old-policy pass (ClippedPPOAgent.RECORD_WHILE_ACTING; 1 = default)")
    ap.add_argument("--conv-dw-one-launch", type=int, default=None, choices=[0, 1],
                    help="A/B: the three convolution weight gradients as one launch (rlx_conv_dw_multi) or three")
    ap.add_argument("--conv-dw-u8", type=int, default=None, choices=[0, 1],
                    help="A/B: conv1's weight gradient by rlx_conv_dw_u8 (frame rows + the image's dz in LDS) or by rlx_gemm")
    ap.add_argument("--conv-fwd-groups", type=int, default=None, choices=[0, 4],
                    help="A/B: wave groups per K slab of the fused forward convolutions (0: the tiled launches' rule, 4: always four)")
    ap.add_argument("--conv32-tail16", type=int, default=None, choices=[0, 1],
                    help="A/B: 16-row tail tiles (v_mfma_f32_16x16x4_f32, two chains per wave) in the fused input-gradient chain")
    ap.add_argument("--conv32-prefetch", type=int, default=None, choices=[1, 2],
                    help="A/B: jobs ahead a wave of the fused input-gradient chain requests its weight operands")
    ap.add_argument("--conv-dw-passes", type=int, default=None, choices=[1, 2, 4],
                    help="A/B: the one-launch convolution weight gradients with operands staged in one / two passes")
    ap.add_argument("--split-cap", type=int, default=None, help="A/B: rlx_gemm_split_cap (most K chunks per product; default 64)")
    ap.add_argument("--heads-row-local", type=int, default=None, choices=[0, 1],
                    help="A/B: the row-local part of the discrete heads inside the last dense layer's reduction, the rest on the "
                         "deferred-reduction launch (rlx_ppo_fc_rows; default on)")
    ap.add_argument("--fc-heads", type=int, default=None, choices=[0, 1],
                    help="A/B: the last dense layer + heads + losses + heads' backward as one launch (rlx_ppo_fc_heads)")
    ap.add_argument("--fuse-conv-bwd", type=int, default=None, choices=[0, 1],
                    help="A/B: the input gradients of conv3 / conv2 as one launch (nn.graph.FUSE_CONV_INPUT_GRADS; 0 = default)")
    ap.add_argument("--fuse-conv-bwd-min-wg", type=int, default=None,
                    help="A/B: fewest half-image workgroups for which the fused input-gradient chain is taken "
                         "(nn.graph.FUSE_CONV_INPUT_GRADS_MIN_WORKGROUPS)")
    ap.add_argument("--update-chunk", type=int, default=None,
                    help="A/B (c4 / c5): consecutive updates of a train() call per captured graph (VectorOffPolicyAgent.UPDATE_CHUNK; "
                         "default 8, 1 = every update on its own)")
    ap.add_argument("--host-draws-ahead", type=int, default=None, choices=[0, 1],
                    help="A/B (c4 / c5): the host-RNG side of Agent.train on a producer thread (VectorOffPolicyAgent.HOST_DRAWS_AHEAD)")
    ap.add_argument("--conv-dw-pairs", type=int, default=None, choices=[0, 1, 2],
                    help="A/B: image pairs per workgroup of the conv2 / conv3 weight gradients (rlx_conv_dw_pairs_per_workgroup)")
    ap.add_argument("--kw-min-tiles", type=int, default=None,
                    help="A/B: rlx_gemm_desc.kw_min_tiles of the dense layers' input gradients (fewest 32-row tiles for which K is "
                         "split over the waves of a workgroup instead of over workgroups + a reduce launch; default 96, "
                         "0 = the library's 192)")
    ap.add_argument("--conv1-chunks", type=int, default=None, choices=[1, 3],
                    help="A/B: accumulator chains of conv1 in the fused forward launch (nn.graph.CONV1_CHUNKS)")
    ap.add_argument("--ppo-chunk", type=int, default=None,
                    help="A/B (c2): rows per forward pass of Clipped PPO's whole-dataset passes (ClippedPPOAgent.DATASET_CHUNK)")
    ap.add_argument("--episode-length", type=int, default=EP_LEN,
                    help="c2: length of the synthetic episodes.  32 (default): every episode closes on the 2048-step "
                         "rollout boundary.  1024 (SURVEY.md 8(d)'s Atari-like length): act_for_full_episodes makes a "
                         "step 65 536 env-steps, V(s) / GAE run over all of them, the 320 updates train on dataset[:2048]")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher / rendezvous / reduction plumbing only (no GPU, gloo): what the CPU "
                         "test of the N-rank entry point runs")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # bare `python bench.py --gpus N`: become the launcher — one rank per GPU on this node
        import socket
        with socket.socket() as s_:
            s_.bind(("127.0.0.1", 0))
            port = s_.getsockname()[1]
        import subprocess
        sys.exit(subprocess.call([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                                  "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
                                  "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]))

    from coach_amd.distributed import GradientSync
    if args.dry_run:
        return dry_run(args)
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP hot path has no CPU fallback")
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = GradientSync(force=args.force_dist)
    if args.sac_branches is not None:
        from coach_amd.agents.soft_actor_critic_agent import SoftActorCriticAgent
        SoftActorCriticAgent.parallel_branches = bool(args.sac_branches)
    if args.ppo_chunk is not None:
        from coach_amd.agents.clipped_ppo_agent import ClippedPPOAgent
        ClippedPPOAgent.DATASET_CHUNK = args.ppo_chunk
    if args.direct_conv_dx is not None:
        from coach_amd.nn import graph as _G3
        _G3.DIRECT_CONV_INPUT_GRAD = {"0": False, "1": True, "always": "always"}[args.direct_conv_dx]
    if args.big_tiles is not None:
        from coach_amd import _rlx as _r
        _r.lib().gemm_big_tiles(args.big_tiles)
    if args.multi_dw is not None:
        from coach_amd.nn import graph as _G2
        _G2.MULTI_DW = bool(args.multi_dw)
    if args.conv23_depth is not None:
        from coach_amd import _rlx
        _rlx.lib().conv23_depth(args.conv23_depth, args.conv23_step)
    if args.fuse_conv is not None:
        from coach_amd.nn import graph as _G
        _G.FUSE_CONV_PAIR, _G.FUSE_CONV_FIRST = args.fuse_conv >= 1, args.fuse_conv >= 2
    if args.record_acting is not None:
        from coach_amd.agents.clipped_ppo_agent import ClippedPPOAgent as _A2
        _A2.RECORD_WHILE_ACTING = bool(args.record_acting)
    if args.fuse_acting is not None:
        from coach_amd.agents.clipped_ppo_agent import ClippedPPOAgent as _A
        _A.FUSE_ACTING_LAUNCHES = bool(args.fuse_acting)
    if args.conv_dw_one_launch is not None:
        from coach_amd.nn import graph as _G3
        _G3.CONV_DW_ONE_LAUNCH = bool(args.conv_dw_one_launch)
    if args.conv_dw_u8 is not None:
        from coach_amd.nn import graph as _G2
        _G2.CONV_DW_U8 = bool(args.conv_dw_u8)
    if args.conv_fwd_groups is not None:
        from coach_amd.nn import graph as _G4
        _G4.CONV_FORWARD_WAVE_GROUPS = args.conv_fwd_groups or None
    if args.conv32_tail16 is not None:
        from coach_amd import _rlx as _R2
        _R2.lib().conv32_tail_tiles(int(args.conv32_tail16))
    if args.conv32_prefetch is not None:
        from coach_amd import _rlx as _R3
        _R3.lib().conv32_prefetch(int(args.conv32_prefetch))
    if args.conv_dw_passes is not None:
        from coach_amd import _rlx as _R4
        _R4.lib().conv_dw_passes(int(args.conv_dw_passes))
    if args.split_cap is not None:
        from coach_amd import _rlx as _R
        _R.lib().gemm_split_cap(int(args.split_cap))
    if args.heads_row_local is not None:
        from coach_amd.nn.networks import ClippedPPONet as _N2
        _N2.HEADS_ROW_LOCAL = bool(args.heads_row_local)
    if args.fc_heads is not None:
        from coach_amd.nn.networks import ClippedPPONet as _N
        _N.FC_HEADS_ONE_LAUNCH = bool(args.fc_heads)
    if args.fuse_conv_bwd is not None:
        from coach_amd.nn import graph as _G
        _G.FUSE_CONV_INPUT_GRADS = bool(args.fuse_conv_bwd)
    if args.update_chunk is not None:
        from coach_amd.agents.vector_agent import VectorOffPolicyAgent as _V2
        _V2.UPDATE_CHUNK = int(args.update_chunk)
    if args.host_draws_ahead is not None:
        from coach_amd.agents.vector_agent import VectorOffPolicyAgent as _V
        _V.HOST_DRAWS_AHEAD = bool(args.host_draws_ahead)
    if args.conv_dw_pairs is not None:
        from coach_amd import _rlx as _R7
        _R7.lib().conv_dw_pairs_per_workgroup(int(args.conv_dw_pairs))
    if args.kw_min_tiles is not None:
        from coach_amd.nn import graph as _G6
        _G6.DENSE_DX_KW_MIN_TILES = int(args.kw_min_tiles)
    if args.conv1_chunks is not None:
        from coach_amd.nn import graph as _G5
        _G5.CONV1_CHUNKS = int(args.conv1_chunks)
    if args.fuse_conv_bwd_min_wg is not None:
        from coach_amd.nn import graph as _G
        _G.FUSE_CONV_INPUT_GRADS_MIN_WORKGROUPS = int(args.fuse_conv_bwd_min_wg)
    if args.gemm_pipeline is not None:
        from coach_amd import _rlx
        _rlx.lib().gemm_pipeline(args.gemm_pipeline)
    if dist.world_size != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, dist.world_size))
    if args.workload != "c2":
        run_off_policy(args, device, dist)
        return
    agent = build_agent(device, dist, ep_len=args.episode_length)
    for _ in range(args.warmup):
        one_step(agent)
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    sampler = LoadSampler(min(3.0, 0.06 * args.steps)) if dist.rank == 0 and args.full and not args.no_roofline else None
    t0 = time.perf_counter()
    for _ in range(args.steps):
        res = one_step(agent)
    torch.cuda.synchronize()
    dist.barrier()
    torch.cuda.synchronize()
    elapsed = dist.max_over_ranks(time.perf_counter() - t0)
    agent.networks["main"].check_status()
    if args.dump_outputs and dist.rank == 0:
        # per-epoch means of [surrogate, entropy, kl, policy-head total, value loss, grad norm, ...] of the last step
        dump_outputs(args.dump_outputs, agent, {"epoch_losses": torch.stack(res)})

    n_updates = EPOCHS * (PLAYING_STEPS // BATCH)
    steps_per_iter = N_ENV * agent.steps_per_phase      # = PLAYING_STEPS when the episodes close on the rollout boundary
    env_steps = dist.world_size * steps_per_iter * args.steps
    out = {
        "metric": "env-steps/sec (+ grad-updates/sec) on Atari-like Clipped-PPO, 64 vectorized envs/GPU",
        "value": round(env_steps / elapsed, 1), "unit": "env-steps/s", "n_gpus": dist.world_size,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
        "data": "synthetic",
        "grad_updates_per_s": round(n_updates * args.steps / elapsed, 1),
        "config": {"workload": "C2: Atari-Pong-like Clipped-PPO, %d vectorized envs/GPU, 84x84x4 uint8 obs, "
                               "GAE(0.99,0.95), rollout %d env-steps (episodes of %d%s), %d epochs x %d "
                               "minibatches of %d, fp32 conv torso x2 (value/policy), TF1-Adam"
                               % (N_ENV, steps_per_iter, args.episode_length,
                                  "" if steps_per_iter == PLAYING_STEPS else
                                  ": act_for_full_episodes plays until every episode is complete, V(s) and GAE over the "
                                  "whole dataset, training on dataset[:%d]" % PLAYING_STEPS,
                                  EPOCHS, PLAYING_STEPS // BATCH, BATCH),
                   "global_env_steps_per_step": dist.world_size * steps_per_iter,
                   "parallelism": "dp%d (env vectors sharded per GPU, flat fp32 gradient all-reduce)"
                                  % dist.world_size,
                   "hip_graphs": bool(agent.use_graphs)},
        "final_losses": {k: float(v) for k, v in agent.signals.items()},
    }
    if dist.enabled and args.full:
        # what the collective path looked like in this run, so that a SCALE line explains itself: ranks as the
        # process group reports them, whether the all-reduce is a node of the update's graph, one gradient all-reduce
        # of the update's size timed on its own (device time, back to back)
        import torch.distributed as tdist
        net = agent.networks["main"]
        us = dist.all_reduce_us(net.params.grads.numel())
        out["rccl"] = {"backend": dist.backend(), "world_size": tdist.get_world_size(), "graph_resident": dist.capturable(),
                       "overlap_two_buckets": bool(agent.overlap_allreduce),
                       "overlap_decision": agent.overlap_decision,      # measured at the first training phase; None = forced
                       "probe_note": dist.probe_note,
                       "gradient_bytes": 4 * net.params.grads.numel(),
                       "late_bucket_bytes": 4 * (net.params.grads.numel() - net.late_gradient_offset()),
                       "allreduce_us": None if us is None else round(us, 1),
                       "allreduces_per_step": n_updates * (2 if agent.overlap_allreduce else 1)}
    if dist.rank == 0 and args.full and not args.no_roofline:
        roof, shapes = gemm_roofline(agent)
        out["roofline"] = roof
        out["box"] = box_calibration(device)
        out["box"]["under_load"] = sampler.result() if sampler else None
        # the one number that separates the pool's box classes on identical code: the first convolution's forward
        # product (uint8 frames, cold operands) as it runs INSIDE the update — 19 us on fast-class boxes, 31 us on slow
        conv1 = [k for k in roof["update_kernels"] if k["kernel"].startswith("gemm_fast_kernel") and
                 k["kernel"].endswith("true, true, false, true>")]
        if conv1:
            out["box"]["conv1_forward_in_update_us"] = conv1[0]["avg_us"]
        # (with conv1 inside the fused forward launch that kernel is gone from the update: the fused launch is the probe)
        fused = [k for k in roof["update_kernels"] if k["kernel"].startswith("conv23_forward_kernel")]
        if fused:
            out["box"]["fused_conv_forward_in_update_us"] = fused[0]["avg_us"]
        if args.shapes:
            for s in shapes:
                print(json.dumps(s), file=sys.stderr)
    if dist.rank == 0 and dist.world_size == 1 and args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline()
        # the REFERENCE's own ClippedPPOAgent code path (kind "reference") cannot run here — /root/reference
        # exists only in the build container — so its committed timing rides along with its provenance
        # (tools/time_reference_cpu_c2.py: real rl_coach agent / memory / filters, numpy network stand-in)
        ref = {}
        # (round 3 files: BASELINE.md section 3 protocol — 1024 env-steps per repetition, median of 5 — and the minibatch
        # updates of the timed phase counted correctly; the round-2 files divided a whole phase by ONE update)
        for key, fn in (("one_core", "r03_cpu_reference_c2_1core.json"), ("all_cores", "r03_cpu_reference_c2.json")):
            try:
                with open(os.path.join(ROOT, "profiles", fn)) as f:
                    r = json.load(f)
                ref[key] = {k: r[k] for k in ("value", "unit", "grad_updates_per_s", "cores", "kind", "where", "sample")}
            except (OSError, ValueError, KeyError):
                pass
        if ref:
            out["cpu_baseline"]["reference"] = ref
    finish(dist, out)


def finish(dist, out):
    """rank 0's ONE JSON line, as the LAST thing on stdout: the process group is torn down first and the C library's
    stdout buffer flushed (RCCL prints its version banner through it — left alone it would land behind the JSON)."""
    if dist.enabled:
        import torch.distributed as tdist
        if tdist.is_initialized():
            dist.barrier()
            tdist.destroy_process_group()
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:
        pass
    sys.stdout.flush()
    if dist.rank == 0:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
