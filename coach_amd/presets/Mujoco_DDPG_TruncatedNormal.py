"""DDPG with the TruncatedNormal exploration policy on the device Pendulum-v0 level.

The agent of rl_coach/presets/Mujoco_DDPG.py (its defaults, 1000 heat-up steps, an evaluation episode every 20 episodes)
with the Ornstein-Uhlenbeck process swapped for rl_coach/exploration_policies/truncated_normal.py: the action is drawn
from the normal distribution around the actor's output restricted to the action bounds, so no probability mass piles
up on them.  MuJoCo itself is not part of this engine; Pendulum-v0 is the bounded continuous-control level whose
simulator runs on the device (coach_amd/environments/classic_control_vector_environment.py), torque in [-2, 2].  The
noise is 10 % of the action range, falling to 2 % over NOISE[2] acting steps; 5 % in evaluation.
"""
from coach_amd.agents.ddpg_agent import DDPGAgentParameters
from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps, TrainingSteps
from coach_amd.environments.gym_environment import GymVectorEnvironment
from coach_amd.exploration_policies.truncated_normal import TruncatedNormalParameters
from coach_amd.graph_managers.basic_rl_graph_manager import BasicRLGraphManager, ScheduleParameters
from coach_amd.schedules import LinearSchedule

NOISE = (0.1, 0.02, 20000)
CLIP = (-2.0, 2.0)            # Pendulum-v0's torque bounds


def make(num_envs=None, agent_seed=0, noise=NOISE):
    schedule = ScheduleParameters()
    schedule.improve_steps = TrainingSteps(10000000000)
    schedule.steps_between_evaluation_periods = EnvironmentEpisodes(20)
    schedule.evaluation_steps = EnvironmentEpisodes(1)
    schedule.heatup_steps = EnvironmentSteps(1000)

    agent = DDPGAgentParameters()
    agent.seed = agent_seed
    agent.exploration = TruncatedNormalParameters()
    agent.exploration.noise_schedule = LinearSchedule(*noise)
    agent.exploration.clip_low, agent.exploration.clip_high = CLIP

    env = GymVectorEnvironment(level='Pendulum-v0')
    if num_envs is not None:
        env.num_envs = num_envs
    return BasicRLGraphManager(agent_params=agent, env_params=env, schedule_params=schedule)


graph_manager = make()
