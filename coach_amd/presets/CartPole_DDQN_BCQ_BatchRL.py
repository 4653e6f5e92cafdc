"""CartPole DDQN-BCQ in Batch RL for the device engine.

The experiment of rl_coach/presets/CartPole_DDQN_BCQ_BatchRL.py, field by field.  A DQN agent (CartPole_DQN's
hyper-parameters: discount .99, a target copy every 100 env-steps, one update per env-step, lr 2.5e-4, MSE loss, epsilon
1 -> 0.01 over 10 k steps) collects a 10 000-transition episodic dataset: 1 000 heat-up steps and 9 000 training steps.
The DDQN-BCQ agent then learns from the frozen dataset (40 % of it is the training set) in epochs of batches of 128:
discount .98, a target copy every 100 updates, lr 1e-4, MSE loss, L2 regularization 1e-4, the kNN action mask with its
defaults, rewards rescaled by 1 / 200 (the trained agent's input filter serves the collecting agent too), 30
reward-model epochs (lr 1e-4, no L2), greedy evaluation over 10 episodes after every epoch.  Its golden test: an evaluation reward of 150 within 50 epochs.  The level is CartPole-v0 on the device
(coach_amd/environments/cartpole_vector_environment.py).  make(off_policy_evaluation=True) adds what the reference preset
sets for its off-policy evaluators: softmax_temperature = 0.2 on the `main` and `reward_model` wrappers, and the graph
manager's switch (IPS, DM, DR, sequential DR and WIS after every epoch, in that epoch's CSV row).  It is off by default:
the module-level graph_manager is the experiment as it was.  make(action_drop="nn") drops actions by the reference's
second method instead: NNImitationModelParameters with the imitation-model wrapper of the reference preset's text (a
ClassificationHead on Dense 1024-1024-512-512-256 and 128-64, lr 1e-4, no L2); the default "knn" sets no
such wrapper and is the experiment as it was.  make(dataset=path) trains on a logged CSV file instead of collecting (there is no
collecting agent then, and the environment only evaluates); with_environment=False runs without a simulator at all, from
the spaces definition of CartPole: the epochs' rows then carry the off-policy estimates and no evaluation reward.
"""
from copy import deepcopy

from coach_amd.agents.ddqn_bcq_agent import DDQNBCQAgentParameters, KNNParameters, NNImitationModelParameters
from coach_amd.architectures.head_parameters import ClassificationHeadParameters
from coach_amd.architectures.layers import Dense
from coach_amd.agents.dqn_agent import DQNAgentParameters
from coach_amd.base_parameters import PresetValidationParameters, VisualizationParameters
from coach_amd.core_types import CsvDataset, EnvironmentEpisodes, EnvironmentSteps, TrainingSteps
from coach_amd.environments.cartpole_vector_environment import CartPoleVectorEnvironmentParameters
from coach_amd.filters.filter import InputFilter
from coach_amd.filters.reward import RewardRescaleFilter
from coach_amd.graph_managers.batch_rl_graph_manager import BatchRLGraphManager
from coach_amd.graph_managers.graph_manager import ScheduleParameters
from coach_amd.memories.episodic.episodic_experience_replay import EpisodicExperienceReplayParameters
from coach_amd.memories.memory import MemoryGranularity
from coach_amd.schedules import LinearSchedule
from coach_amd.spaces import DiscreteActionSpace, ObservationSpace, SpacesDefinition, StateSpace

DATASET_SIZE = 10000


def make(seed=1234, agent_seed=0, dataset_size=DATASET_SIZE, heatup_steps=1000, reward_model_num_epochs=30,
         improve_epochs=10000000000, batch_size=128, evaluation_episodes=10, train_to_eval_ratio=0.4,
         off_policy_evaluation=False, dataset=None, with_environment=True, action_drop="knn"):
    """seed: the environment's reset-state streams; agent_seed: both agents' host generators and initial weights;
    off_policy_evaluation: the five off-policy estimates after every epoch (softmax_temperature 0.2);
    dataset: the path of a CSV file of logged transitions (core_types.CsvDataset) the trained agent's memory starts as;
    with_environment: False — no simulator (needs a dataset);
    action_drop: "knn" — the kNN action mask; "nn" — the imitation model's mask (NNImitationModelParameters)"""
    if action_drop not in ("knn", "nn"):
        raise ValueError('action_drop is "knn" or "nn", got %r' % (action_drop,))
    sched = ScheduleParameters()
    sched.improve_steps = TrainingSteps(improve_epochs)
    sched.steps_between_evaluation_periods = TrainingSteps(1)
    sched.evaluation_steps = EnvironmentEpisodes(evaluation_episodes)
    sched.heatup_steps = EnvironmentSteps(dataset_size)

    agent = DDQNBCQAgentParameters()
    agent.seed = agent_seed
    main = agent.network_wrappers['main']
    main.batch_size = batch_size
    agent.algorithm.num_steps_between_copying_online_weights_to_target = TrainingSteps(100)
    agent.algorithm.discount = 0.98
    agent.algorithm.action_drop_method_parameters = KNNParameters()
    agent.input_filter = InputFilter()
    agent.input_filter.add_reward_filter('rescale', RewardRescaleFilter(1 / 200.))
    main.learning_rate = 0.0001
    main.replace_mse_with_huber_loss = False
    main.l2_regularization = 0.0001
    agent.network_wrappers['reward_model'] = deepcopy(main)
    agent.network_wrappers['reward_model'].learning_rate = 0.0001
    agent.network_wrappers['reward_model'].l2_regularization = 0
    if action_drop == "nn":
        agent.algorithm.action_drop_method_parameters = NNImitationModelParameters()
        im = agent.network_wrappers['imitation_model'] = deepcopy(main)
        im.learning_rate, im.l2_regularization = 0.0001, 0
        im.heads_parameters = [ClassificationHeadParameters()]
        im.input_embedders_parameters['observation'].scheme = [Dense(1024), Dense(1024), Dense(512), Dense(512), Dense(256)]
        im.middleware_parameters.scheme = [Dense(128), Dense(64)]
    if off_policy_evaluation:
        main.softmax_temperature = 0.2
        agent.network_wrappers['reward_model'].softmax_temperature = 0.2
    agent.memory = EpisodicExperienceReplayParameters()
    if dataset is not None:
        agent.memory.load_memory_from_file_path = CsvDataset(dataset)
    agent.exploration.epsilon_schedule = LinearSchedule(0, 0, 10000)
    agent.exploration.evaluation_epsilon = 0

    gen = DQNAgentParameters()
    gen.seed = agent_seed
    gen_sched = ScheduleParameters()
    gen_sched.heatup_steps = EnvironmentSteps(heatup_steps)
    gen_sched.improve_steps = TrainingSteps(dataset_size - heatup_steps)
    gen_sched.steps_between_evaluation_periods = EnvironmentEpisodes(10)
    gen_sched.evaluation_steps = EnvironmentEpisodes(1)
    gen.algorithm.num_steps_between_copying_online_weights_to_target = EnvironmentSteps(100)
    gen.algorithm.discount = 0.99
    gen.algorithm.num_consecutive_playing_steps = EnvironmentSteps(1)
    gen.network_wrappers['main'].learning_rate = 0.00025
    gen.network_wrappers['main'].replace_mse_with_huber_loss = False
    gen.memory = EpisodicExperienceReplayParameters()
    gen.memory.max_size = (MemoryGranularity.Transitions, dataset_size)
    gen.exploration.epsilon_schedule = LinearSchedule(1.0, 0.01, 10000)

    env = CartPoleVectorEnvironmentParameters(1, "CartPole-v0", seed=seed) if with_environment else None
    spaces = None if with_environment else SpacesDefinition(
        state=StateSpace({'observation': ObservationSpace(4)}), goal=None, action=DiscreteActionSpace(2))
    validation = PresetValidationParameters(test=True, min_reward_threshold=150, max_episodes_to_achieve_reward=50,
                                            read_csv_tries=500)
    if dataset is not None:                  # nothing is collected: the file is the dataset
        gen = gen_sched = None
    manager = BatchRLGraphManager(agent_params=agent, experience_generating_agent_params=gen,
                                  experience_generating_schedule_params=gen_sched, env_params=env, schedule_params=sched,
                                  vis_params=VisualizationParameters(dump_signals_to_csv_every_x_episodes=1),
                                  preset_validation_params=validation, reward_model_num_epochs=reward_model_num_epochs,
                                  train_to_eval_ratio=train_to_eval_ratio, spaces_definition=spaces)
    if off_policy_evaluation:
        manager.off_policy_evaluation = True
    return manager


graph_manager = make()
