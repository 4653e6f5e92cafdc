#!/usr/bin/env python
"""Generate tests/golden/pg.npz by running the REFERENCE's own PolicyGradientsAgent code under the stub-import harness
(_refstub.py), in the manner of make_golden_c51.py.  Run from the repo root in the build container (the reference tree
must be present):

    python tests/golden/make_golden_pg.py

Recorded:
  * runs of consecutive episodes through PolicyOptimizationAgent.train, update_episode_statistics and
    PolicyGradientsAgent.learn_from_batch with a stand-in network that records what accumulate_gradients received (the
    states' indices, the actions, the fp64 targets) and when apply_gradients_and_sync_networks fired: every one of the
    four rescalers at discounts 0.99 and 1.0 with whole-episode windows, and two runs with
    num_steps_between_gradient_updates = 5 (windows that start in the middle of an episode).  The driver feeds train()
    the way the level manager does: the transition of a non-terminal step enters the episode buffer at the start of the
    NEXT step, a terminal one at once, and current_episode is incremented (handle_episode_ended) before train();
    after every window: the two per-timestep statistics arrays, the signals' samples, current_episode and
    training_iteration;
  * Categorical.get_action in TRAIN and TEST on a few probability rows (two with tied maxima), with np.random's state
    before and after;
  * the parameter classes' defaults (JSON text under "defaults").
Rewards are fp32-exact (the device keeps filtered rewards as fp32) and not all equal.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refstub  # noqa: E402

_refstub.install()

from rl_coach.agents.policy_optimization_agent import PolicyGradientRescaler  # noqa: E402
from rl_coach.core_types import Episode, RunPhase, Transition  # noqa: E402
from rl_coach.spaces import DiscreteActionSpace  # noqa: E402

# lengths: 1, 2, 7, 8, 9; 3 is shorter than all before it; 7, 8, 9, 12, 16 are each longer than all before them
LENGTHS = (5, 3, 7, 8, 9, 2, 1, 12, 4, 9, 16, 6, 1)
STAT_LEN = 24                                                # entries of the statistics arrays that are recorded
RESCALERS = ("TOTAL_RETURN", "FUTURE_RETURN", "FUTURE_RETURN_NORMALIZED_BY_EPISODE",
             "FUTURE_RETURN_NORMALIZED_BY_TIMESTEP")
# (rescaler, discount, num_steps_between_gradient_updates)
RUNS = tuple((r, d, 20000) for r in RESCALERS for d in (0.99, 1.0)) + \
    (("FUTURE_RETURN_NORMALIZED_BY_TIMESTEP", 0.99, 5), ("TOTAL_RETURN", 0.99, 5))
N_ACTIONS = 3


class _Obj(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


class _Samples(object):
    def __init__(self):
        self.values = []

    def add_sample(self, v):
        self.values.append(float(v))


def _fake_agent(rescaler, discount, t_max, calls):
    from rl_coach.agents.policy_gradients_agent import PolicyGradientsAgent

    class Fake(PolicyGradientsAgent):
        def __init__(self):
            pass

        def post_training_commands(self):
            pass
    f = Fake()
    wrapper = _Obj(input_embedders_parameters={'observation': None})
    f.ap = _Obj(network_wrappers={'main': wrapper},
                algorithm=_Obj(discount=discount, num_steps_between_gradient_updates=t_max,
                               apply_gradients_every_x_episodes=5, policy_gradient_rescaler=rescaler))
    f.policy_gradient_rescaler = rescaler
    f.last_gradient_update_step_idx = 0
    f.max_episode_length = 100000
    f.mean_return_over_multiple_episodes = np.zeros(f.max_episode_length)
    f.num_episodes_where_step_has_been_seen = np.zeros(f.max_episode_length)
    f.returns_mean, f.returns_variance = _Samples(), _Samples()
    f.spaces = _Obj(action=DiscreteActionSpace(N_ACTIONS))
    f.current_episode, f.training_iteration = 0, 0

    def accumulate(inputs, targets):
        calls.append(dict(idx=np.array(inputs['observation']).reshape(-1).astype(np.int64),
                          actions=np.array(inputs['output_0_0']).astype(np.int64),
                          targets=np.array(targets, dtype=np.float64), applied=False))
        return 0.0, [0.0], 0.0

    def apply():
        calls[-1]["applied"] = True
    f.networks = {'main': _Obj(online_network=_Obj(accumulate_gradients=accumulate), set_is_training=lambda s: None,
                               apply_gradients_and_sync_networks=apply)}
    return f


def gen_runs(out, rng):
    for r, (name, discount, t_max) in enumerate(RUNS):
        calls = []
        f = _fake_agent(PolicyGradientRescaler[name], discount, t_max, calls)
        rewards_all, actions_all, g = [], [], 0
        for L in LENGTHS:
            rewards = rng.uniform(-1.0, 2.0, size=L).astype(np.float32)
            actions = rng.randint(0, N_ACTIONS, size=L)
            rewards_all.append(rewards)
            actions_all.append(actions)
            f.current_episode_buffer = Episode(discount=discount, n_step=-1)
            pending = None
            for t in range(L):
                if pending is not None:                      # the previous response is observed now (level_manager.py:236)
                    f.current_episode_buffer.insert(pending)
                    pending = None
                tr = Transition(state={'observation': np.array([g])}, action=int(actions[t]), reward=float(rewards[t]),
                                next_state={'observation': np.array([g + 1])}, game_over=t == L - 1)
                g += 1
                if t == L - 1:                               # a terminal response is observed at once (:260-264)
                    f.current_episode_buffer.insert(tr)
                    f.current_episode += 1                   # handle_episode_ended (agent.py:572-573)
                else:
                    pending = tr
                before = len(calls)
                f.train()
                if len(calls) > before:
                    c = calls[-1]
                    c["mean"] = f.mean_return_over_multiple_episodes[:STAT_LEN].copy()
                    c["seen"] = f.num_episodes_where_step_has_been_seen[:STAT_LEN].copy()
                    c["current_episode"], c["training_iteration"] = f.current_episode, f.training_iteration
                    c["episode_mean"] = float(getattr(f, "mean_discounted_return", 0.0))
                    c["episode_std"] = float(getattr(f, "std_discounted_return", 0.0))
        assert f.mean_return_over_multiple_episodes[STAT_LEN:].max() == 0 and max(LENGTHS) <= STAT_LEN
        p = "r%d_" % r
        out[p + "lengths"] = np.array(LENGTHS)
        out[p + "rewards"] = np.concatenate(rewards_all)
        out[p + "actions"] = np.concatenate(actions_all)
        out[p + "discount"], out[p + "t_max"] = np.float64(discount), np.int64(t_max)
        out[p + "rescaler"] = np.int64(PolicyGradientRescaler[name].value)
        out[p + "win_first"] = np.array([c["idx"][0] for c in calls])        # global index of the window's first state
        out[p + "win_len"] = np.array([c["idx"].size for c in calls])
        assert all(np.array_equal(c["idx"], c["idx"][0] + np.arange(c["idx"].size)) for c in calls)
        out[p + "win_actions"] = np.concatenate([c["actions"] for c in calls])
        out[p + "targets"] = np.concatenate([c["targets"] for c in calls])   # fp64, as handed to accumulate_gradients
        out[p + "applied"] = np.array([c["applied"] for c in calls])
        out[p + "current_episode"] = np.array([c["current_episode"] for c in calls])
        out[p + "training_iteration"] = np.array([c["training_iteration"] for c in calls])
        out[p + "mean"] = np.stack([c["mean"] for c in calls])
        out[p + "seen"] = np.stack([c["seen"] for c in calls])
        out[p + "episode_mean"] = np.array([c["episode_mean"] for c in calls])
        out[p + "episode_std"] = np.array([c["episode_std"] for c in calls])
        out[p + "returns_mean"] = np.array(f.returns_mean.values)
        out[p + "returns_variance"] = np.array(f.returns_variance.values)
        print("run %d %s discount %s t_max %d: %d windows, %d applies" % (r, name, discount, t_max, len(calls),
                                                                          int(out[p + "applied"].sum())))


def gen_categorical(out, rng):
    from rl_coach.exploration_policies.categorical import Categorical
    rows = rng.dirichlet(np.ones(4), size=6).astype(np.float32)
    rows[1] = [0.4, 0.4, 0.1, 0.1]                          # tied maxima: np.argmax takes the first
    rows[4] = [0.1, 0.3, 0.3, 0.3]
    np.random.seed(1234)
    state0 = np.random.get_state()
    pol = Categorical(DiscreteActionSpace(4))                # no draw on construction
    assert np.array_equal(np.random.get_state()[1], state0[1]) and np.random.get_state()[2] == state0[2]
    pol.phase = RunPhase.TRAIN
    train = [int(pol.get_action(p)[0]) for p in rows]
    state1 = np.random.get_state()
    pol.phase = RunPhase.TEST
    test = [int(pol.get_action(p)[0]) for p in rows]
    state2 = np.random.get_state()
    assert np.array_equal(state1[1], state2[1]) and state1[2] == state2[2]
    out["cat_probs"], out["cat_train"], out["cat_test"] = rows, np.array(train), np.array(test)
    out["cat_seed"] = np.int64(1234)
    out["cat_state_after_keys"], out["cat_state_after_pos"] = state1[1].copy(), np.int64(state1[2])


def gen_defaults(out):
    from rl_coach.agents.policy_gradients_agent import PolicyGradientsAgentParameters
    ap = PolicyGradientsAgentParameters()
    net, alg = ap.network_wrappers['main'], ap.algorithm
    d = {"policy_gradient_rescaler": alg.policy_gradient_rescaler.name,
         "apply_gradients_every_x_episodes": alg.apply_gradients_every_x_episodes, "beta_entropy": alg.beta_entropy,
         "num_steps_between_gradient_updates": alg.num_steps_between_gradient_updates, "discount": alg.discount,
         "learning_rate": net.learning_rate, "optimizer_type": net.optimizer_type,
         "optimizer_epsilon": net.optimizer_epsilon, "adam_optimizer_beta1": net.adam_optimizer_beta1,
         "adam_optimizer_beta2": net.adam_optimizer_beta2, "clip_gradients": net.clip_gradients,
         "async_training": net.async_training, "create_target_network": net.create_target_network,
         "head": type(net.heads_parameters[0]).__name__, "heads": len(net.heads_parameters),
         "embedder_scheme": net.input_embedders_parameters['observation'].scheme.name,
         "middleware_scheme": net.middleware_parameters.scheme.name,
         "activation_function": net.middleware_parameters.activation_function,
         "classes": [type(alg).__name__, type(net).__name__, type(ap).__name__],
         "discrete_exploration": type(ap.exploration[DiscreteActionSpace]).__name__,
         "memory": type(ap.memory).__name__,
         "rescalers": {r.name: r.value for r in PolicyGradientRescaler}}
    out["defaults"] = np.array(json.dumps(d, sort_keys=True))


def main():
    rng = np.random.RandomState(77)
    out = {}
    gen_runs(out, rng)
    gen_categorical(out, rng)
    gen_defaults(out)
    path = os.path.join(HERE, "pg.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.1f KiB)" % (path, len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
