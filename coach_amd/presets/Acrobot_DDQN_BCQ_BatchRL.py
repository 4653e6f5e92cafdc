"""Acrobot DDQN-BCQ in Batch RL for the device engine.

The experiment of rl_coach/presets/Acrobot_DDQN_BCQ_BatchRL.py, field by field, built like CartPole_DDQN_BCQ_BatchRL.  A
Double DQN agent (discount .99, a target copy every 100 env-steps, one update per env-step, lr 1e-4, batches of 128, MSE
loss, epsilon 1 -> 0.01 over the dataset) collects a 50 000-transition episodic dataset: 1 000 heat-up steps and 49 000
training steps.  The DDQN-BCQ agent then learns from the frozen dataset (40 % of it is the training set) in epochs of
batches of 128: discount .99, a target copy every 100 updates, lr 1e-4, MSE loss, the kNN action mask with its defaults,
softmax_temperature 0.2, 30 reward-model epochs, greedy evaluation over 10 episodes after every epoch.  Both Q heads start
from an output bias of -100 (`QHeadParameters(output_bias_initializer=-100)`, the reference's
tf.constant_initializer(-100)): an Acrobot return is -500 at worst and a step costs -1, so a fresh network starts
pessimistic rather than at 0, which lies above every real return.  The reference's validation numbers (150 within 50 epochs) are copied as they
stand; an Acrobot reward never reaches them.  The level is Acrobot-v1 on the device
(coach_amd/environments/classic_control_vector_environment.py).
"""
from coach_amd.agents.ddqn_agent import DDQNAgentParameters
from coach_amd.agents.ddqn_bcq_agent import DDQNBCQAgentParameters, KNNParameters
from coach_amd.architectures.head_parameters import QHeadParameters
from coach_amd.base_parameters import PresetValidationParameters, VisualizationParameters
from coach_amd.core_types import EnvironmentEpisodes, EnvironmentSteps, TrainingSteps
from coach_amd.environments.classic_control_vector_environment import AcrobotVectorEnvironmentParameters
from coach_amd.graph_managers.batch_rl_graph_manager import BatchRLGraphManager
from coach_amd.graph_managers.graph_manager import ScheduleParameters
from coach_amd.memories.episodic.episodic_experience_replay import EpisodicExperienceReplayParameters
from coach_amd.memories.memory import MemoryGranularity
from coach_amd.schedules import LinearSchedule

DATASET_SIZE = 50000
OUTPUT_BIAS = -100.0


def make(seed=1234, agent_seed=0, dataset_size=DATASET_SIZE, heatup_steps=1000, reward_model_num_epochs=30,
         improve_epochs=10000000000, batch_size=128, evaluation_episodes=10, train_to_eval_ratio=0.4):
    """seed: the environment's reset-state streams; agent_seed: both agents' host generators and initial weights"""
    sched = ScheduleParameters()
    sched.improve_steps = TrainingSteps(improve_epochs)
    sched.steps_between_evaluation_periods = TrainingSteps(1)
    sched.evaluation_steps = EnvironmentEpisodes(evaluation_episodes)
    sched.heatup_steps = EnvironmentSteps(dataset_size)

    agent = DDQNBCQAgentParameters()
    agent.seed = agent_seed
    main = agent.network_wrappers['main']
    main.batch_size = batch_size
    main.heads_parameters = [QHeadParameters(output_bias_initializer=OUTPUT_BIAS)]
    agent.algorithm.num_steps_between_copying_online_weights_to_target = TrainingSteps(100)
    agent.algorithm.discount = 0.99
    agent.algorithm.action_drop_method_parameters = KNNParameters()
    main.learning_rate = 0.0001
    main.replace_mse_with_huber_loss = False
    main.softmax_temperature = 0.2
    agent.memory = EpisodicExperienceReplayParameters()
    agent.exploration.epsilon_schedule = LinearSchedule(0, 0, 10000)
    agent.exploration.evaluation_epsilon = 0

    gen = DDQNAgentParameters()
    gen.seed = agent_seed
    gen_sched = ScheduleParameters()
    gen_sched.heatup_steps = EnvironmentSteps(heatup_steps)
    gen_sched.improve_steps = TrainingSteps(dataset_size - heatup_steps)
    gen_sched.steps_between_evaluation_periods = EnvironmentEpisodes(10)
    gen_sched.evaluation_steps = EnvironmentEpisodes(1)
    gen.algorithm.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(100)
    gen.algorithm.discount = 0.99
    gen.algorithm.num_consecutive_playing_steps = EnvironmentSteps(1)
    gen_main = gen.network_wrappers['main']
    gen_main.learning_rate = 0.0001
    gen_main.batch_size = batch_size
    gen_main.replace_mse_with_huber_loss = False
    gen_main.heads_parameters = [QHeadParameters(output_bias_initializer=OUTPUT_BIAS)]
    gen.memory = EpisodicExperienceReplayParameters()
    gen.memory.max_size = (MemoryGranularity.Transitions, dataset_size + 1)
    gen.exploration.epsilon_schedule = LinearSchedule(1.0, 0.01, dataset_size)
    gen.exploration.evaluation_epsilon = 0

    validation = PresetValidationParameters(test=True, min_reward_threshold=150, max_episodes_to_achieve_reward=50,
                                            read_csv_tries=500)
    return BatchRLGraphManager(agent_params=agent, experience_generating_agent_params=gen,
                               experience_generating_schedule_params=gen_sched,
                               env_params=AcrobotVectorEnvironmentParameters(1, seed=seed), schedule_params=sched,
                               vis_params=VisualizationParameters(dump_signals_to_csv_every_x_episodes=1),
                               preset_validation_params=validation, reward_model_num_epochs=reward_model_num_epochs,
                               train_to_eval_ratio=train_to_eval_ratio)


graph_manager = make()
