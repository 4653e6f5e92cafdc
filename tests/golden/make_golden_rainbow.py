#!/usr/bin/env python
"""Generate tests/golden/rainbow.npz by running the REFERENCE's own Rainbow code under the stub-import harness
(_refstub.py), in the manner of make_golden_c51.py.  Run from the repo root in the build container (the reference tree
must be present):

    python tests/golden/make_golden_rainbow.py

Recorded:
  * RainbowDQNAgent.learn_from_batch with stand-in networks: online_network.predict returns fixed fp32 softmaxes (the
    Double-DQN choice), parallel_prediction the target's and the online ones, train_and_sync_networks records its targets
    and returns fp64 cross entropies, and the memory is a PrioritizedExperienceReplay whose update_priorities call is
    recorded — the C51 generator's four shapes, one of them with the support [0, 200] and returns up to 3 rewards of 1;
    ~30 % of the rows have should_bootstrap_next_state False.  The device sums an action's expectation in atom order
    while numpy's dot may not: a row whose two largest online Q values on s' are closer than 1e-6 is redrawn (fewer
    than 1 % of the rows, asserted);
  * Episode(n_step=3).update_transitions_rewards_and_bootstrap_data for T = 1, 2, 3, 4 and 7: the returns, the flags and
    which state every next_state is;
  * a PrioritizedExperienceReplay of 16 leaves being stored such episodes one after the other (the store loop of
    agent.py:582-583), sampled after the third and — past the ring's end — after the fifth, with priority updates in
    between: leaves and weights for recorded random.random() draws, the payload order, num_transitions();
  * the parameter classes' defaults (JSON text under "defaults").
"""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstub  # noqa: E402

_refstub.install()

from rl_coach.core_types import Batch, Episode, Transition  # noqa: E402
from rl_coach.memories.memory import MemoryGranularity  # noqa: E402
from rl_coach.memories.non_episodic.prioritized_experience_replay import PrioritizedExperienceReplay  # noqa: E402
from rl_coach.schedules import ConstantSchedule  # noqa: E402

from make_golden_c51 import CASES, MIN_GAP, _Obj, _softmax32  # noqa: E402

DISCOUNT, N_STEP = 0.99, 3
EPISODE_LENGTHS = (1, 2, 3, 4, 7)
STORED_LENGTHS = (4, 7, 3, 1, 2)             # 17 transitions into 16 leaves


def _fake_agent(N, v_min, v_max):
    from rl_coach.agents.rainbow_dqn_agent import RainbowDQNAgent

    class Fake(RainbowDQNAgent):
        def __init__(self):
            pass

    class FakeMemory(PrioritizedExperienceReplay):
        def __init__(self):
            pass
    f = Fake()
    wrapper = _Obj(input_embedders_parameters={'observation': None})
    f.ap = _Obj(network_wrappers={'main': wrapper},
                algorithm=_Obj(discount=DISCOUNT, n_step=N_STEP, atoms=N, v_min=v_min, v_max=v_max))
    f.z_values = np.linspace(v_min, v_max, N)
    f.q_values = _Obj(add_sample=lambda v: None)
    f.memory = FakeMemory()
    return f


def gen_learn(out, rng):
    total = redrawn = 0
    for s, (B, A, N, v_min, v_max, ones) in enumerate(CASES):
        f = _fake_agent(N, v_min, v_max)
        p_sel = _softmax32(rng, (B, A, N))
        while True:                                          # the condition on the inputs (see the module text)
            q = np.sort(f.distribution_prediction_to_q_values(p_sel), axis=1)
            close = (q[:, -1] - q[:, -2]) < MIN_GAP
            if not close.any():
                break
            p_sel[close] = _softmax32(rng, (int(close.sum()), A, N))
            redrawn += int(close.sum())
        total += B
        p_target, p_online = _softmax32(rng, (B, A, N)), _softmax32(rng, (B, A, N))
        actions = rng.randint(0, A, size=B)
        boot = rng.rand(B) >= 0.3
        if ones:                 # what Episode gives for rewards of 1: 2.9701 inside, 1.99 and 1 at the episode's end
            ep = Episode(discount=DISCOUNT, n_step=N_STEP)
            for _ in range(7):
                ep.insert(Transition(state={'observation': np.zeros(1)}, action=0, reward=1.0,
                                     next_state={'observation': np.zeros(1)}, game_over=False))
            ep.update_transitions_rewards_and_bootstrap_data()
            pick = rng.randint(0, 7, size=B)
            returns = np.array([ep.transitions[i].n_step_discounted_rewards for i in pick])
            boot = np.array([ep.transitions[i].info['should_bootstrap_next_state'] for i in pick])
        else:
            returns = rng.randn(B) * 2
        captured = {}
        main = _Obj(target_network=object(),
                    online_network=_Obj(predict=lambda states: p_sel.copy()),
                    parallel_prediction=lambda pairs: (p_target.copy(), p_online.copy()))

        def train(inputs, targets, importance_weights=None):
            captured['targets'] = np.array(targets)
            captured['importance_weights'] = np.array(importance_weights)
            ce = -(captured['targets'].astype(np.float64) * np.log(p_online.astype(np.float64))).sum(axis=-1)
            captured['losses'] = ce
            return 0.0, [ce], 0.0
        main.train_and_sync_networks = train
        f.networks = {'main': main}
        f.call_memory = lambda name, args: captured.__setitem__(name, args)
        tr = []
        for i in range(B):
            t = Transition(state={'observation': rng.randn(4)}, action=int(actions[i]), reward=1.0,
                           next_state={'observation': rng.randn(4)}, game_over=False,
                           info={'should_bootstrap_next_state': bool(boot[i]), 'idx': i, 'weight': 0.5})
            t.n_step_discounted_rewards = float(returns[i])
            tr.append(t)
        f.learn_from_batch(Batch(tr))
        assert captured['targets'].dtype == np.float32 and captured['importance_weights'].shape == (B,)
        idx, errors = captured['update_priorities']
        assert list(idx) == list(range(B))
        p = "s%d_" % s
        out[p + "p_sel"], out[p + "p_target"], out[p + "p_online"] = p_sel, p_target, p_online
        out[p + "z"], out[p + "actions"], out[p + "returns"], out[p + "boot"] = f.z_values, actions, returns, boot
        out[p + "targets"] = captured['targets']                          # fp32 [B, A, N]
        out[p + "target_actions"] = np.argmax(f.distribution_prediction_to_q_values(p_sel), axis=1)
        out[p + "errors"] = np.asarray(errors, dtype=np.float64)
        out[p + "discount_n"] = np.float64(DISCOUNT ** N_STEP)
        print("case %d %s: %d rows without bootstrap, returns in [%.3f, %.3f]" % (
            s, (B, A, N), int((~boot).sum()), returns.min(), returns.max()))
    assert redrawn < 0.01 * total, (redrawn, total)
    print("%d of %d rows redrawn" % (redrawn, total))


def _episode(T, rng, first_id):
    """an Episode of T transitions whose states carry ids first_id .. first_id + T - 1; the last next state has id
    -(first_id + T)."""
    ep = Episode(discount=DISCOUNT, n_step=N_STEP)
    for k in range(T):
        nxt = first_id + k + 1 if k < T - 1 else -(first_id + T)
        ep.insert(Transition(state={'observation': np.array([first_id + k])}, action=k % 2,
                             reward=float(np.float32(rng.randn())), next_state={'observation': np.array([nxt])},
                             game_over=k == T - 1))
    return ep


def gen_episodes(out, rng):
    for T in EPISODE_LENGTHS:
        ep = _episode(T, rng, 100)
        rewards = np.array([t.reward for t in ep.transitions], dtype=np.float32)
        ep.update_transitions_rewards_and_bootstrap_data()
        p = "ep%d_" % T
        out[p + "rewards"] = rewards
        out[p + "returns"] = np.array([t.n_step_discounted_rewards for t in ep.transitions], dtype=np.float64)
        out[p + "boot"] = np.array([t.info['should_bootstrap_next_state'] for t in ep.transitions])
        # which state the next state is: the index of the transition whose STATE it is, or T for the last next state
        ids = np.array([int(t.next_state['observation'][0]) for t in ep.transitions])
        out[p + "next"] = np.where(ids < 0, T, ids - 100)


def _sample(mem, size, seed):
    random.seed(seed)
    u = np.array([random.random() for _ in range(size)])
    random.seed(seed)
    batch = mem.sample(size)
    return u, np.array([t.info['idx'] for t in batch]), np.array([t.info['weight'] for t in batch]), \
        np.array([int(t.state['observation'][0]) for t in batch])


def gen_memory(out, rng):
    mem = PrioritizedExperienceReplay((MemoryGranularity.Transitions, 16), alpha=0.5, beta=ConstantSchedule(0.4))
    first, rewards, counts = 0, [], []
    for e, T in enumerate(STORED_LENGTHS):
        ep = _episode(T, rng, first)
        rewards.append(np.array([t.reward for t in ep.transitions], dtype=np.float32))
        ep.update_transitions_rewards_and_bootstrap_data()
        for t in ep.transitions:                       # agent.py:582-583
            mem.store(t)
        first += T
        counts.append(mem.num_transitions())
        if e in (2, 4):
            p = "mem%d_" % e
            out[p + "u"], out[p + "idx"], out[p + "weight"], out[p + "state_ids"] = _sample(mem, 8, 10 + e)
            err = np.abs(rng.randn(8))
            mem.update_priorities(out[p + "idx"], err)
            out[p + "errors"] = err
            out[p + "u2"], out[p + "idx2"], out[p + "weight2"], out[p + "state_ids2"] = _sample(mem, 8, 20 + e)
            out[p + "max_priority"] = np.float64(mem.maximal_priority)
            out[p + "sum_total"] = np.float64(mem.sum_tree.total_value())
    out["mem_rewards"] = np.concatenate(rewards)
    out["mem_lengths"] = np.array(STORED_LENGTHS)
    out["mem_num_transitions"] = np.array(counts)
    out["mem_order"] = np.array([int(t.state['observation'][0]) for t in mem.transitions])   # the payload, oldest first


def gen_defaults(out):
    from rl_coach.agents.rainbow_dqn_agent import RainbowDQNAgentParameters
    ap = RainbowDQNAgentParameters()
    net = ap.network_wrappers['main']
    d = {"atoms": ap.algorithm.atoms, "v_min": ap.algorithm.v_min, "v_max": ap.algorithm.v_max,
         "n_step": ap.algorithm.n_step,
         "store_transitions_only_when_episodes_are_terminated":
             ap.algorithm.store_transitions_only_when_episodes_are_terminated,
         "discount": ap.algorithm.discount, "learning_rate": net.learning_rate,
         "optimizer_epsilon": net.optimizer_epsilon, "batch_size": net.batch_size,
         "head": type(net.heads_parameters[0]).__name__,
         "middleware_scheme": str(getattr(net.middleware_parameters.scheme, "name", net.middleware_parameters.scheme)),
         "classes": [type(ap.algorithm).__name__, type(ap.exploration).__name__, type(net).__name__],
         "num_steps_between_copying_online_weights_to_target":
             ap.algorithm.num_steps_between_copying_online_weights_to_target.num_steps,
         "num_consecutive_playing_steps": ap.algorithm.num_consecutive_playing_steps.num_steps,
         "memory": type(ap.memory).__name__, "alpha": ap.memory.alpha, "epsilon": ap.memory.epsilon,
         "beta": [type(ap.memory.beta).__name__, float(ap.memory.beta.current_value)],
         "max_size": int(ap.memory.max_size[1])}
    out["defaults"] = np.array(json.dumps(d, sort_keys=True))


def main():
    rng = np.random.RandomState(63)
    out = {}
    gen_learn(out, rng)
    gen_episodes(out, rng)
    gen_memory(out, rng)
    gen_defaults(out)
    path = os.path.join(HERE, "rainbow.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.1f KiB)" % (path, len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
