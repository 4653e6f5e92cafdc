"""The parameters class under this module's name keeps refusing, as tests/test_c51_ref.py and tests/test_qr_dqn_ref.py
pin it.  Rainbow DQN itself is coach_amd/agents/rainbow_agent.py, and the import layer (coach_amd.compat) serves the
reference's module path rl_coach.agents.rainbow_dqn_agent from there, so that the reference's preset texts — those that
use the agent (presets/CartPole_Rainbow.py) and those that only import the name (presets/CartPole_QR_DQN.py, line 2) —
run unchanged.
"""


class RainbowDQNAgentParameters(object):
    def __init__(self):
        raise NotImplementedError("Rainbow DQN (noisy nets, the n-step prioritized replay and the dueling head over "
                                  "atoms) is coach_amd.agents.rainbow_agent.RainbowDQNAgentParameters; the class of "
                                  "this name in coach_amd.agents.rainbow_dqn_agent builds nothing")
