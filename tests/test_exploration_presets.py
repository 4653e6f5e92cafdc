"""The Boltzmann / TruncatedNormal / Greedy policies from the public side: presets, the reference-idiom imports, the
refusal of an agent that does not serve them, and the schedules over a short run on the device."""
import numpy as np
import pytest


def test_the_presets_build_their_parameters_and_the_reference_imports_resolve():
    import coach_amd.compat as compat
    from coach_amd.presets import CartPole_DQN_Boltzmann, Mujoco_DDPG_TruncatedNormal
    b = CartPole_DQN_Boltzmann.graph_manager.agent_params.exploration
    t = Mujoco_DDPG_TruncatedNormal.graph_manager.agent_params.exploration
    assert (b.temperature_schedule.initial_value, b.temperature_schedule.final_value) == (1.0, 0.01)
    assert b.path.endswith("boltzmann:Boltzmann") and t.path.endswith("truncated_normal:TruncatedNormal")
    assert (t.clip_low, t.clip_high, t.evaluation_noise, t.noise_as_percentage_from_action_space) == (-2.0, 2.0, 0.05, True)
    compat.install()
    try:
        from rl_coach.exploration_policies.boltzmann import BoltzmannParameters
        from rl_coach.exploration_policies.greedy import GreedyParameters
        from rl_coach.exploration_policies.truncated_normal import TruncatedNormalParameters
        d = TruncatedNormalParameters()                               # the reference's defaults (:31-35)
        assert (d.clip_low, d.clip_high, d.evaluation_noise, d.noise_schedule.current_value) == (0, 1, 0.05, 0.1)
        assert type(b) is BoltzmannParameters and GreedyParameters().path.endswith("greedy:Greedy")
    finally:
        compat.uninstall()


def test_an_agent_that_does_not_serve_the_policy_refuses_it_by_name():
    from coach_amd.agents.soft_actor_critic_agent import SoftActorCriticAgent, SoftActorCriticAgentParameters
    from coach_amd.exploration_policies import BoltzmannParameters
    params = SoftActorCriticAgentParameters()
    params.exploration = BoltzmannParameters()
    with pytest.raises(ValueError, match="Boltzmann exploration is served for DQNAgent.* not for SoftActorCriticAgent"):
        SoftActorCriticAgent(params, None)


def _stepped(schedule_args, steps):
    from coach_amd.schedules import LinearSchedule
    s = LinearSchedule(*schedule_args)
    for _ in range(steps):
        s.step()
    return s.current_value


@pytest.mark.gpu
@pytest.mark.parametrize("preset", ["CartPole_DQN_Boltzmann", "Mujoco_DDPG_TruncatedNormal"])
def test_a_preset_runs_and_its_schedule_moves_in_train_only(dev, preset):
    import importlib
    from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps
    mod = importlib.import_module("coach_amd.presets." + preset)
    boltzmann = preset.endswith("Boltzmann")
    gm = mod.make(num_envs=4, temperature=(1.0, 0.01, 100)) if boltzmann else mod.make(num_envs=4, noise=(0.1, 0.02, 400))
    gm.env_params.episode_length = 25
    gm.device = dev
    gm.create_graph()
    pol = gm.agent.exploration_policy
    gm.heatup(EnvironmentSteps(40))                                   # random actions: the policy is not asked
    assert np.all(pol.get_control_param() == (1.0 if boltzmann else 0.1))
    gm.train_and_act(EnvironmentSteps(160))                           # 40 vector steps of 4 envs
    # Boltzmann steps its temperature once per acting step; TruncatedNormal its noise once per env, as AdditiveNoise
    want = _stepped((1.0, 0.01, 100), 40) if boltzmann else _stepped((0.1, 0.02, 400), 160)
    assert gm.agent.training_iteration > 0 and np.all(pol.get_control_param() == want) and want < (1.0 if boltzmann else 0.1)
    gm.evaluate(EnvironmentEpisodes(1))                               # TEST: the schedule stands still
    assert np.all(pol.get_control_param() == want)
    gm.agent.check_status()
    if not boltzmann:
        a = gm.agent.actions.cpu().numpy()
        assert (a >= -2.0).all() and (a <= 2.0).all()
