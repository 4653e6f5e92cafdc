"""Learning with Bootstrapped DQN (slow, GPU): the CartPole_Bootstrapped_DQN preset on the device CartPole against the bar
the reference sets for its CartPole DQN-family presets: an averaged evaluation reward of 150 within 250 episodes, agent
seed 0.  The bar is applied as tests/test_cartpole.py applies CartPole_DQN's."""
import importlib

import pytest


@pytest.mark.gpu
def test_cartpole_bootstrapped_dqn_preset_reaches_the_golden_threshold(dev, tmp_path):
    import torch
    name = "CartPole_Bootstrapped_DQN"
    gm = importlib.import_module("coach_amd.presets." + name).make(agent_seed=0)
    gm.device = dev
    gm.logger.__init__(str(tmp_path / (name + ".csv")))
    st = gm.run_preset_validation(time_limit=15 * 60)
    gm.environment.check_status()
    net = gm.agent.networks["main"]
    assert net.K == 10 and torch.isfinite(net.params.weights).all()
    print("%s: %s at episode %d of %d (best averaged evaluation reward %.1f, %.0f s, %d training iterations)" % (
        name, st["reason"], st["episode"], st["max_episodes_to_achieve_reward"], st["averaged_rewards"].max(),
        st["wall_s"], gm.agent.training_iteration))
    assert st["passed"], st
