"""CartPole Mixed Monte Carlo for the device engine — a preset of this package, not one of the reference's (its only
Mixed Monte Carlo preset is Doom_Health_MMC, a level this engine does not serve).

CartPole_PAL's experiment with the MixedMonteCarloAgent in the PAL agent's place: discount .99, a target copy every
100 env-steps, one update per env-step, lr 2.5e-4, MSE loss, a 40 k-transition episodic replay, epsilon 1 -> 0.01 over
10 k steps, 1 000 heat-up steps, one evaluation episode every 10 episodes, Monte Carlo mixing rate 0.1.  This preset
has NO reference bar: the validation parameters repeat the family's 150 within 250 episodes so that the graph manager
can report against them, but no reference preset states that number for this agent and no test asserts it.
"""
from coach_amd.agents.mmc_agent import MixedMonteCarloAgentParameters
from coach_amd.presets import CartPole_PAL


def make(num_envs=1, seed=1234, agent_seed=0, **overrides):
    return CartPole_PAL.make(num_envs=num_envs, seed=seed, agent_seed=agent_seed,
                             agent_parameters=MixedMonteCarloAgentParameters, **overrides)


graph_manager = make()
