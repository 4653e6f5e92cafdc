"""PAL and Mixed Monte Carlo on the CPU: the numpy restatement (tests/pal_ref.py) against what the reference's own
PALAgent (plain and persistent) and MixedMonteCarloAgent computed (tests/golden/pal_mmc.npz, make_golden_pal_mmc.py) and
against the oracle's Double-DQN targets; the package's parameter defaults and its CartPole_PAL preset against the
reference's (pal_mmc.npz "defaults", tests/golden/pal_preset.json); the import layer; the C ABI entry."""
import importlib
import json
import os
import re

import numpy as np
import pytest

import pal_ref as R
from test_preset_dropin import REF, _exec_preset, needs_reference

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = {"s0": (32, 2), "s1": (37, 6), "s2": (5, 18), "tie": (10, 4)}       # (B, A)
MODES = ("pal", "ppal", "mmc")                                              # ppal: persistent


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "pal_mmc.npz"))


def case(gold, name):
    keys = ("q_sel", "q_next", "q_cur", "q_online", "actions", "rewards", "go", "total_returns", "discount", "alpha",
            "rate", "redrawn") + tuple("targets_" + m for m in MODES)
    return {k: gold[name + "_" + k] for k in keys}


def ref_targets(c, mode, alpha=None, rate=None):
    return R.targets(c["q_online"], None if mode == "mmc" else c["q_cur"], c["q_next"], c["q_sel"], c["actions"],
                     c["rewards"], c["go"], c["total_returns"], float(c["discount"]),
                     float(c["alpha"]) if alpha is None else alpha, mode == "ppal",
                     float(c["rate"]) if rate is None else rate)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_targets_equal_the_reference_agents_bit_for_bit(gold, name, mode):
    c = case(gold, name)
    B, A = CASES[name]
    want = c["targets_" + mode]
    assert want.shape == (B, A) and want.dtype == np.float32 and c["total_returns"].dtype == np.float64
    assert c["rewards"].dtype == np.float32 and int(c["redrawn"]) >= 0
    td = ref_targets(c, mode)
    assert td.dtype == np.float32 and np.array_equal(td.view(np.uint32), want.view(np.uint32))
    other = np.ones((B, A), bool)
    other[np.arange(B), c["actions"]] = False
    assert np.array_equal(td[other], c["q_online"][other])                 # only the taken action changes


def test_the_golden_cases_hold_what_they_are_meant_to_hold(gold):
    for name in ("s0", "s1", "s2"):
        c = case(gold, name)
        assert c["go"].any() and not c["go"].all()
        for k in ("q_sel", "q_next", "q_cur"):                              # no argmax hangs on the last bits
            top = np.sort(c[k], axis=1)
            assert (top[:, -1] - top[:, -2]).min() >= 1e-6
        # the three agents do differ, and the persistent form differs from the plain one somewhere
        assert not np.array_equal(c["targets_pal"], c["targets_mmc"])
        assert not np.array_equal(c["targets_pal"], c["targets_ppal"])
    c = case(gold, "tie")
    rows = np.arange(10)
    sel = np.argmax(c["q_sel"], axis=1)
    adv = c["q_cur"].max(axis=1) - c["q_cur"][rows, c["actions"]]
    adv_next = c["q_next"].max(axis=1) - c["q_next"][rows, sel]
    tied = lambda q: (q == q.max(axis=1, keepdims=True)).sum(axis=1) > 1
    assert tied(c["q_sel"])[[0, 1, 3, 9]].all() and sel[:2].tolist() == [1, 0] and sel[3] == 2
    assert tied(c["q_cur"])[[2, 5, 9]].all() and tied(c["q_next"])[[3, 9]].all()
    assert (adv[[4, 5]] == 0).all() and (adv > 0).sum() >= 5
    assert (adv_next[[6, 7]] < adv[[6, 7]]).all() and adv_next[6] == 0 and adv_next[7] > 0
    assert adv_next[8] == adv[8] > 0
    # where min picks the next state's advantage the two forms differ; where the advantage is 0 they are equal
    differ = c["targets_pal"][rows, c["actions"]] != c["targets_ppal"][rows, c["actions"]]
    assert differ[[6, 7]].all() and not differ[[4, 5, 8]].any()


@pytest.mark.parametrize("name", ["s0", "s1"])
def test_the_goldens_decide_between_fp32_and_fp64_products(gold, name):
    """numpy 1.x's value-based casting made `alpha * min(...)` and `(1 - rate) * TD_targets[i, a]` fp64 products; the
    recorded targets (numpy >= 2) are not reproduced by that arithmetic."""
    c = case(gold, name)
    B = len(c["actions"])
    alpha, rate, g = float(c["alpha"]), float(c["rate"]), float(c["discount"])
    td = c["q_online"].copy()
    for i in range(B):
        a, sel = c["actions"][i], np.argmax(c["q_sel"][i])
        td[i, a] = np.float64(c["rewards"][i]) + (1.0 - c["go"][i]) * g * np.float64(c["q_next"][i][sel])
        td[i, a] = np.float64(td[i, a]) - alpha * np.float64(np.float32(c["q_cur"][i].max() - c["q_cur"][i][a]))
        td[i, a] = (1 - rate) * np.float64(td[i, a]) + rate * c["total_returns"][i]
    assert not np.array_equal(td.view(np.uint32), c["targets_pal"].view(np.uint32))
    np.testing.assert_allclose(td, c["targets_pal"], rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_without_correction_and_mix_the_targets_are_the_oracles_double_dqn_targets(gold, name, mode):
    from oracle.targets import dqn_targets
    c = case(gold, name)
    td = ref_targets(c, mode, alpha=0.0, rate=0.0)
    want, _ = dqn_targets(c["q_next"], c["q_online"], c["actions"], c["rewards"], c["go"], float(c["discount"]),
                          q_next_online=c["q_sel"])
    assert want.dtype == np.float32 and np.array_equal(td.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("huber", [True, False])
def test_loss_restatement_equals_torch_autograd_of_the_head_loss(gold, huber):
    torch = pytest.importorskip("torch")
    c = case(gold, "s1")
    B, A = CASES["s1"]
    u = R.update(c["q_online"], c["q_cur"], c["q_next"], c["q_sel"], c["actions"], c["rewards"], c["go"],
                 c["total_returns"], 0.99, 0.7, True, 0.3, huber)
    q = torch.tensor(c["q_online"], dtype=torch.float64, requires_grad=True)
    t = torch.tensor(u["td_targets"], dtype=torch.float64)
    per = torch.nn.functional.huber_loss(q, t, reduction="none") if huber else (q - t) ** 2
    loss = per.sum(dim=1).mean()                                 # head.py:172-181
    loss.backward()
    np.testing.assert_allclose(u["loss"], loss.item(), rtol=2e-6)
    np.testing.assert_allclose(u["dq"], q.grad.numpy(), rtol=2e-6, atol=1e-9)
    assert R.tree_leaves(1) == 64 and R.tree_leaves(64) == 64 and R.tree_leaves(65) == 128 and R.tree_leaves(1024) == 1024


def _defaults(ap):
    net = ap.network_wrappers['main']
    sch = ap.exploration.epsilon_schedule
    alg = ap.algorithm
    return {
        "algorithm": {k: getattr(alg, k) for k in ("pal_alpha", "persistent_advantage_learning",
                                                   "monte_carlo_mixing_rate", "discount") if hasattr(alg, k)},
        "classes": [type(ap).__name__, type(alg).__name__, type(ap.exploration).__name__, type(ap.memory).__name__],
        "learning_rate": net.learning_rate, "optimizer_epsilon": net.optimizer_epsilon,
        "batch_size": net.batch_size, "replace_mse_with_huber_loss": net.replace_mse_with_huber_loss,
        "head": type(net.heads_parameters[0]).__name__,
        "epsilon_schedule": [type(sch).__name__, float(sch.initial_value), float(sch.final_value),
                             int(sch.decay_steps)],
        "evaluation_epsilon": ap.exploration.evaluation_epsilon,
        "agent_path": ap.path, "memory_path": ap.memory.path,
        "memory_max_size": [ap.memory.max_size[0].name, int(ap.memory.max_size[1])],
        "n_step": ap.memory.n_step,
        "num_steps_between_copying_online_weights_to_target":
            alg.num_steps_between_copying_online_weights_to_target.num_steps,
        "num_consecutive_playing_steps": alg.num_consecutive_playing_steps.num_steps}


def test_parameter_defaults_equal_the_reference(gold):
    from coach_amd.agents.mmc_agent import MixedMonteCarloAgentParameters
    from coach_amd.agents.pal_agent import PALAgentParameters
    ref = json.loads(str(gold["defaults"]))
    assert _defaults(PALAgentParameters()) == ref["pal"]
    assert _defaults(MixedMonteCarloAgentParameters()) == ref["mmc"]
    assert ref["pal"]["algorithm"] == {"pal_alpha": 0.9, "persistent_advantage_learning": False,
                                       "monte_carlo_mixing_rate": 0.1, "discount": 0.99}
    assert "pal_alpha" not in ref["mmc"]["algorithm"] and ref["mmc"]["algorithm"]["monte_carlo_mixing_rate"] == 0.1


def test_reference_module_paths_resolve_through_the_import_layer():
    import coach_amd.compat as compat
    compat.install()
    pal = importlib.import_module("rl_coach.agents.pal_agent")
    mmc = importlib.import_module("rl_coach.agents.mmc_agent")
    import coach_amd.agents.mmc_agent as mine_mmc
    import coach_amd.agents.pal_agent as mine_pal
    for name in ("PALAlgorithmParameters", "PALAgentParameters", "PALAgent"):
        assert getattr(pal, name) is getattr(mine_pal, name)
    for name in ("MixedMonteCarloAlgorithmParameters", "MixedMonteCarloAgentParameters", "MixedMonteCarloAgent"):
        assert getattr(mmc, name) is getattr(mine_mmc, name)


def test_cartpole_pal_preset_equals_the_unchanged_reference_preset_text():
    """tests/golden/pal_preset.json holds what the reference's CartPole_PAL.py text, executed unchanged through the
    import layer, set (make_pal_preset_dump.py): the package's preset must equal it field by field."""
    from test_cartpole import _dump
    with open(os.path.join(GOLDEN, "pal_preset.json")) as f:
        ref = json.load(f)["CartPole_PAL"]
    mine = importlib.import_module("coach_amd.presets.CartPole_PAL").graph_manager
    assert ref["level_name"] == "CartPole-v0" and mine.env_params.level == "CartPole-v0"
    for part in ("agent_params", "schedule", "preset_validation_params"):
        assert ref[part] == _dump(getattr(mine, part)), part
    ap = mine.agent_params
    assert type(ap).__name__ == "PALAgentParameters" and type(ap.memory).__name__ == "EpisodicExperienceReplayParameters"
    assert ap.network_wrappers["main"].learning_rate == 0.00025
    assert ap.network_wrappers["main"].replace_mse_with_huber_loss is False
    assert ap.memory.max_size[1] == 40000 and ap.algorithm.num_consecutive_playing_steps.num_steps == 1
    assert ap.algorithm.num_steps_between_copying_online_weights_to_target.num_steps == 100
    s = ap.exploration.epsilon_schedule
    assert (s.initial_value, s.final_value, s.decay_steps) == (1.0, 0.01, 10000)
    assert mine.schedule.heatup_steps.num_steps == 1000
    v = mine.preset_validation_params
    assert v.test and v.min_reward_threshold == 150 and v.max_episodes_to_achieve_reward == 250


def test_cartpole_mmc_preset_is_the_same_experiment_with_the_mmc_agent():
    from test_cartpole import _dump
    mmc = importlib.import_module("coach_amd.presets.CartPole_MMC")
    mine, pal = mmc.graph_manager, importlib.import_module("coach_amd.presets.CartPole_PAL").graph_manager
    assert "NO reference bar" in mmc.__doc__
    assert type(mine.agent_params).__name__ == "MixedMonteCarloAgentParameters"
    assert _dump(mine.schedule) == _dump(pal.schedule)
    assert _dump(mine.agent_params.memory) == _dump(pal.agent_params.memory)
    assert _dump(mine.agent_params.exploration) == _dump(pal.agent_params.exploration)
    assert _dump(mine.agent_params.network_wrappers["main"]) == _dump(pal.agent_params.network_wrappers["main"])
    a, b = _dump(mine.agent_params.algorithm), _dump(pal.agent_params.algorithm)
    for k in ("__class__", "pal_alpha", "persistent_advantage_learning"):
        a.pop(k, None), b.pop(k, None)
    assert a == b


@needs_reference
def test_reference_preset_text_builds_a_graph_manager_unchanged():
    from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager
    ns = _exec_preset(open(os.path.join(REF, "CartPole_PAL.py")).read())
    gm = ns["graph_manager"]
    assert isinstance(gm, BasicRLGraphManager) and gm.agent_params is ns["agent_params"]
    assert type(gm.agent_params).__module__ == "coach_amd.agents.pal_agent"
    assert gm.agent_params.path == "coach_amd.agents.pal_agent:PALAgent"


def test_noisy_layers_and_unknown_modes_are_refused():
    from coach_amd.nn.networks import MixedTargetDQNNet
    with pytest.raises(ValueError, match="noisy"):
        MixedTargetDQNNet("cpu", (4,), 2, noisy=True)
    assert MixedTargetDQNNet.FUSED_MLP is False and MixedTargetDQNNet.FUSED_ACT is False
    assert MixedTargetDQNNet.HEAD_FORWARD_WITH_TORSO is False and MixedTargetDQNNet.MODES == ("pal", "mmc")


def test_abi_declares_the_entry_point():
    from coach_amd import _rlx
    protos = _rlx.parse_header()
    names = [n for _, n in protos["rlx_mixed_target_head_loss"][1]]
    assert names == ["q_online", "ld_q", "q_target_cur", "q_next_target", "q_next_selector", "ld_next", "actions",
                     "rewards", "game_overs", "total_returns", "discount", "pal_alpha", "persistent", "mixing_rate",
                     "batch", "n_actions", "huber", "grad_scale", "dq", "ld_dq", "td_targets", "ld_targets",
                     "loss_scalar", "status", "stream"]
    src = open(os.path.join(ROOT, "coach_amd", "csrc", "pal.hip")).read()
    assert re.search(r"\bint\s+rlx_mixed_target_head_loss\s*\(", src)
    assert "atomicAdd" not in src and src.count("atomic") == 1           # the status flag alone
    assert "(float)pal_alpha" in src and "(float)(1.0 - mixing_rate)" in src
    mk = open(os.path.join(ROOT, "coach_amd", "csrc", "Makefile")).read()
    assert "pal" in mk.split("EXACT :=")[1].split("$(foreach")[0].split()
    assert _rlx.ABI_VERSION == 11
