from .boltzmann import Boltzmann, BoltzmannParameters
from .greedy import Greedy, GreedyParameters
from .truncated_normal import TruncatedNormal, TruncatedNormalParameters

# Which agents take these three (the reference's base classes would hand them to any agent of the matching action
# space; here a policy is served where the agent's acting step forms what it reads): Boltzmann and the discrete Greedy
# read ONE row of Q values per env, TruncatedNormal and the box Greedy the deterministic action of an actor.
VALUE_ROW_AGENTS = ("DQNAgent", "DDQNAgent", "PALAgent", "MixedMonteCarloAgent", "NStepQAgent")   # (dueling: a head of these)
ACTOR_MEAN_AGENTS = ("DDPGAgent", "TD3Agent", "NAFAgent")
_SERVED = ((BoltzmannParameters, "Boltzmann", VALUE_ROW_AGENTS),
           (TruncatedNormalParameters, "TruncatedNormal", ACTOR_MEAN_AGENTS),
           (GreedyParameters, "Greedy", VALUE_ROW_AGENTS + ACTOR_MEAN_AGENTS))


def check_exploration_served(agent_name, agent_parameters):
    """refuse, by name and before anything touches the device, an agent that was given one of the policies above but
    does not serve it"""
    p = getattr(agent_parameters, "exploration", None)
    for cls, what, served in _SERVED:
        if isinstance(p, cls) and agent_name not in served:
            raise ValueError("%s exploration is served for %s, not for %s" % (what, ", ".join(served), agent_name))
