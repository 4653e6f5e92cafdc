#!/usr/bin/env python
"""Generate tests/golden/imitation.npz by running the REFERENCE's own imitation code under the stub-import harness
(_refstub.py), in the manner of make_golden_bcq.py.  Run from the repo root where the reference tree is present:

    python tests/golden/make_golden_imitation.py

Recorded:
  * bc_*: BCAgent.learn_from_batch on a batch of B = 5 transitions — the inputs ('observation', 'output_0_0') and the
    targets it hands train_and_sync_networks.
  * act_*: ImitationAgent.choose_action over a fixed list of action-probability rows with the reference's EGreedy
    (epsilon schedule at 1.0 — a TRAIN-phase policy would always explore — and evaluation_epsilon 0.25) after
    np.random.seed(4): the policy's phase after each call and the actions (a restatement replays the decisions on numpy's
    stream from the same seed).
  * <c>_*: per case of CASES (B, A), DDQNBCQAgent.select_actions with NNImitationModelParameters on stand-in networks
    (fixed fp32 outputs): q_sel = online on s', logits of the imitation model, its predict = imitation_ref.softmax_parts
    (tf.nn.softmax is not installed; the stand-in IS the project's definition), and for the case "p" probabilities placed
    by hand.  Stored: mask, zero_rows, selected actions, the rows redrawn.
  * sched<i>_*: improve_reward_model(epochs) with imitation_model_num_epochs = 3 and epochs = 2 and 5 over a memory
    stand-in that yields 3 batches per epoch (sizes 4, 4, 2): which network was trained on which batch in which order
    (0 = reward model, 1 = imitation model; the batch by the reward of its first transition), the one-hot targets of
    every imitation update, how many generators were opened.
  * "defaults": the parameter classes' defaults as JSON text.
Input conditions (as make_golden_bcq.py): a row whose two best unmasked selector values are closer than 1e-6, or one of
whose familiarities is within 1e-6 (relative) of the threshold, is redrawn (at most 5 % of a case's rows; the count is
printed; with Gaussian logits none is expected).  The rows placed by hand are exempt: in every A = 3 case rows 0 and 1
are uniform logits (every probability 1/3 < 0.35: zero-confidence rows), and in the probabilities case "p" row 2 holds
exactly np.float32(0.35) (not masked in fp32; an fp64 comparison would mask it) and row 3 the next fp32 below it (masked).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]
import _refstub  # noqa: E402

_refstub.install()

import imitation_ref  # noqa: E402
from rl_coach.core_types import Batch, RunPhase, Transition  # noqa: E402

CASES = ((1, 2), (5, 3), (37, 18), (128, 3))
THRESHOLD = 0.35
MIN_GAP = 1e-6


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _transitions(rng, B, A, D=4):
    return [Transition(state={'observation': rng.randn(D).astype(np.float32)}, action=int(rng.randint(A)),
                       reward=float(i), next_state={'observation': rng.randn(D).astype(np.float32)}, game_over=False)
            for i in range(B)]


def gen_bc(out):
    from rl_coach.agents.bc_agent import BCAgent

    class Fake(BCAgent):
        def __init__(self):
            pass
    rng = np.random.RandomState(2)
    tr = _transitions(rng, 5, 3)
    captured = {}

    def train(inputs, targets):
        captured["inputs"], captured["targets"] = inputs, np.array(targets)
        return 1.5, [1.5], 0.25
    f = Fake()
    f.ap = _Obj(network_wrappers={'main': _Obj(input_embedders_parameters={'observation': None})})
    f.networks = {'main': _Obj(train_and_sync_networks=train)}
    assert f.learn_from_batch(Batch(tr)) == (1.5, [1.5], 0.25) and f.is_on_policy is False
    assert sorted(captured["inputs"]) == ['observation', 'output_0_0']
    out["bc_observation"] = np.array(captured["inputs"]['observation'])
    out["bc_output_0_0"] = np.array(captured["inputs"]['output_0_0'])
    out["bc_targets"] = captured["targets"]
    out["bc_actions"] = np.array([t.action for t in tr])
    out["bc_states"] = np.array([t.state['observation'] for t in tr])


def gen_choose_action(out):
    from rl_coach.agents.imitation_agent import ImitationAgent
    from rl_coach.exploration_policies.e_greedy import EGreedy
    from rl_coach.schedules import ConstantSchedule
    from rl_coach.spaces import DiscreteActionSpace

    class Fake(ImitationAgent):
        def __init__(self):
            pass
    rng = np.random.RandomState(6)
    A, n = 3, 40
    logits = (rng.randn(n, A) * 2).astype(np.float32)
    probs = imitation_ref.softmax_parts(logits)[0]
    probs[3] = [0.25, 0.5, 0.25]
    probs[4] = [0.5, 0.5, 0.0]                                # a tie: the random tie-break decides
    state = {"i": 0}
    f = Fake()
    f.networks = {'main': _Obj(online_network=_Obj(predict=lambda x: probs[state["i"]][None].copy()))}
    f.prepare_batch_for_inference = lambda s, name: s
    np.random.seed(4)
    f.exploration_policy = EGreedy(DiscreteActionSpace(A), ConstantSchedule(1.0), 0.25)
    assert f.exploration_policy.phase == RunPhase.HEATUP
    f.exploration_policy.change_phase(RunPhase.TRAIN)
    actions, phases = [], []
    for i in range(n):
        state["i"] = i
        a = f.choose_action(None).action
        actions.append(int(a[0] if isinstance(a, tuple) else a))
        phases.append(f.exploration_policy.phase == RunPhase.TEST)
    out["act_probs"], out["act_actions"], out["act_phase_is_test"] = probs, np.array(actions), np.array(phases)
    out["act_evaluation_epsilon"], out["act_schedule_value"] = np.float64(0.25), np.float64(1.0)
    greedy = np.argmax(probs, axis=1)
    out["act_greedy"] = greedy
    print("choose_action: %d of %d actions differ from the greedy one (evaluation_epsilon 0.25 applies: the phase is "
          "forced to TEST)" % (int((np.array(actions) != greedy).sum()), n))
    f2 = Fake()
    try:
        f2.learn_from_batch(None)
        raise SystemExit("ImitationAgent.learn_from_batch did not raise")
    except NotImplementedError as e:
        out["imitation_error"] = np.array(str(e))
    from rl_coach.agents.agent import Agent
    Agent.__init__ = lambda self, agent_parameters, parent=None: None                 # the base constructor is not run
    g = ImitationAgent(None)
    out["imitation_flag"] = np.array(bool(g.imitation))


def fake_bcq_agent(nn, A, networks):
    import rl_coach.agents.ddqn_bcq_agent as mod

    class Fake(mod.DDQNBCQAgent):
        def __init__(self):
            pass
    f = Fake()
    f.ap = _Obj(network_wrappers={'main': _Obj(input_embedders_parameters={'observation': None}),
                                  'reward_model': _Obj(input_embedders_parameters={'observation': None}, batch_size=4)},
                algorithm=_Obj(action_drop_method_parameters=nn))
    f.spaces = _Obj(action=_Obj(actions=list(range(A))))
    f.networks = networks
    return f


def run_select(q_sel, familiarity):
    import rl_coach.agents.ddqn_bcq_agent as mod
    nn = mod.NNImitationModelParameters()
    assert nn.mask_out_actions_threshold == THRESHOLD
    handle = {}

    def predict_q(x):
        handle["masked"] = q_sel.copy()
        return handle["masked"]
    f = fake_bcq_agent(nn, q_sel.shape[1], {
        'imitation_model': _Obj(online_network=_Obj(predict=lambda x: familiarity.copy())),
        'main': _Obj(online_network=_Obj(predict=predict_q))})
    np.random.seed(11)
    selected = np.array(f.select_actions(None, None))
    m = handle["masked"]
    zero = ~np.isneginf(m).any(axis=1) & (m != q_sel).all(axis=1)
    return dict(mask=np.isneginf(m) | zero[:, None], zero_rows=zero, selected=selected)


def settle(rng, q, x, fixed, probs_in):
    """redraw the rows that sit on a decision boundary -> rows redrawn"""
    redrawn = 0
    while True:
        sel, fam, mask, zero = imitation_ref.imitation_selector(q, x, THRESHOLD, probs_in=probs_in)
        bad = []
        for b in range(len(q)):
            if b in fixed:
                continue
            live = np.sort(q[b][~mask[b]])
            close_q = len(live) > 1 and (live[-1] - live[-2]) < MIN_GAP
            close_f = (np.abs(fam[b].astype(np.float64) - THRESHOLD) <= MIN_GAP * THRESHOLD).any()
            if close_q or close_f:
                bad.append(b)
        if not bad:
            return fam, redrawn
        for b in bad:
            q[b] = (rng.randn(q.shape[1]) * 2).astype(np.float32)
            x[b] = imitation_ref.softmax_parts(rng.randn(q.shape[1]))[0] if probs_in else \
                (rng.randn(q.shape[1]) * 1.5).astype(np.float32)
        redrawn += len(bad)


def gen_select(out):
    rng = np.random.RandomState(1812)
    thr32 = np.float32(THRESHOLD)
    assert not (np.array([thr32]) < THRESHOLD)[0] and float(thr32) < THRESHOLD       # fp32 keeps it, fp64 would mask it
    cases = [("n%d" % i, B, A, False) for i, (B, A) in enumerate(CASES)] + [("p", 5, 3, True)]
    for name, B, A, probs_in in cases:
        q = (rng.randn(B, A) * 2).astype(np.float32)
        x = (rng.randn(B, A) * 1.5).astype(np.float32)
        fixed = set()
        if probs_in:
            x = imitation_ref.softmax_parts(x)[0]
            below = np.nextafter(thr32, np.float32(0))
            x[0], x[1] = [0.3, 0.34, 0.34], [0.2, 0.3, 0.3]                  # zero-confidence rows
            x[2] = [thr32, 0.5, np.float32(1) - np.float32(0.5) - thr32]
            x[3] = [below, 0.5, np.float32(1) - np.float32(0.5) - below]
            fixed = {0, 1, 2, 3}
        elif A == 3:
            x[0] = 0
            x[1] = np.float32(2.5)                                           # uniform: every probability 1/3 < 0.35
            fixed = {0, 1}
        fam, redrawn = settle(rng, q, x, fixed, probs_in)
        assert redrawn <= 0.05 * B, "%d of %d rows redrawn" % (redrawn, B)
        r = run_select(q, fam)
        if A == 3:
            assert r["zero_rows"][:2].all()
        if probs_in:
            assert not r["mask"][2, 0] and r["mask"][3, 0] and not r["zero_rows"][2:4].any()
        out[name + "_q_sel"], out[name + "_imitation"], out[name + "_familiarity"] = q, x, fam
        out[name + "_redrawn"] = np.int64(redrawn)
        for k, v in r.items():
            out[name + "_" + k] = v
        print("case %s (B=%d A=%d %s): %d entries masked, %d zero-confidence rows, %d rows redrawn"
              % (name, B, A, "probabilities" if probs_in else "logits", int(r["mask"].sum()), int(r["zero_rows"].sum()),
                 redrawn))


def gen_schedule(out):
    import rl_coach.agents.ddqn_bcq_agent as mod
    mod.screen = _Obj(log_dict=lambda *a, **k: None)
    rng = np.random.RandomState(9)
    A = 3
    tr = _transitions(rng, 10, A)
    for i, epochs in enumerate((2, 5)):
        nn = mod.NNImitationModelParameters()
        nn.imitation_model_num_epochs = 3
        log, targets, opened = [], [], [0]

        def train_imitation(inputs, t):
            log.append((1, int(inputs["first"])))
            targets.append(np.array(t))
            return [0.5]
        f = fake_bcq_agent(nn, A, {'imitation_model': _Obj(train_and_sync_networks=train_imitation)})
        f.get_reward_model_loss = lambda batch: log.append((0, int(batch.rewards()[0]))) or 0.25

        def call_memory(name, size):
            assert name == 'get_shuffled_training_data_generator' and size == 4
            opened[0] += 1
            return iter([tr[0:4], tr[4:8], tr[8:10]])
        f.call_memory = call_memory
        Batch.states_orig = Batch.states
        Batch.states = lambda self, keys: {"first": self.rewards()[0]}
        try:
            f.improve_reward_model(epochs)
        finally:
            Batch.states = Batch.states_orig
            del Batch.states_orig
        p = "sched%d_" % i
        out[p + "epochs"], out[p + "imitation_epochs"] = np.int64(epochs), np.int64(3)
        out[p + "log"], out[p + "generators"] = np.array(log), np.int64(opened[0])
        out[p + "targets"] = np.concatenate(targets)
        out[p + "target_dtype"] = np.array(str(targets[0].dtype))
        print("schedule %d: epochs %d -> %d updates, %d generators" % (i, epochs, len(log), opened[0]))
    out["sched_actions"] = np.array([t.action for t in tr])
    out["sched_batch_firsts"] = np.array([0, 4, 8])
    out["sched_batch_sizes"] = np.array([4, 4, 2])


def gen_defaults(out):
    from rl_coach.agents.bc_agent import BCAgentParameters, BCAlgorithmParameters, BCNetworkParameters
    from rl_coach.agents.ddqn_bcq_agent import NNImitationModelParameters
    from rl_coach.architectures.head_parameters import ClassificationHeadParameters
    ap = BCAgentParameters()
    net, alg = ap.network_wrappers['main'], ap.algorithm
    assert isinstance(net, BCNetworkParameters) and isinstance(alg, BCAlgorithmParameters)
    head = ClassificationHeadParameters()
    sch = ap.exploration.epsilon_schedule
    d = {"classes": [type(ap).__name__, type(alg).__name__, type(ap.exploration).__name__, type(ap.memory).__name__,
                     type(net).__name__],
         "agent_path": ap.path.replace("rl_coach", "coach_amd"),
         "memory_path": ap.memory.path.replace("rl_coach", "coach_amd"),
         "head": type(net.heads_parameters[0]).__name__, "optimizer_type": net.optimizer_type,
         "batch_size": net.batch_size, "replace_mse_with_huber_loss": net.replace_mse_with_huber_loss,
         "create_target_network": net.create_target_network, "learning_rate": net.learning_rate,
         "middleware": [type(net.middleware_parameters).__name__, str(net.middleware_parameters.scheme)],
         "embedders": sorted(net.input_embedders_parameters),
         "has_beta_entropy": hasattr(alg, "beta_entropy"),
         "num_consecutive_playing_steps": [type(alg.num_consecutive_playing_steps).__name__,
                                           alg.num_consecutive_playing_steps.num_steps],
         "epsilon_schedule": [type(sch).__name__, float(sch.initial_value), float(sch.final_value), int(sch.decay_steps)],
         "evaluation_epsilon": ap.exploration.evaluation_epsilon,
         "classification_head": {"name": head.name, "parameterized_class_name": head.parameterized_class_name,
                                 "activation_function": head.activation_function, "loss_weight": head.loss_weight,
                                 "num_output_head_copies": head.num_output_head_copies,
                                 "rescale_gradient_from_head_by_factor": head.rescale_gradient_from_head_by_factor},
         "nn_imitation": dict(vars(NNImitationModelParameters()))}
    out["defaults"] = np.array(json.dumps(d, sort_keys=True))


def main():
    out = {}
    gen_bc(out)
    gen_select(out)
    gen_schedule(out)
    gen_defaults(out)
    gen_choose_action(out)
    path = os.path.join(HERE, "imitation.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.1f KiB)" % (path, len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
