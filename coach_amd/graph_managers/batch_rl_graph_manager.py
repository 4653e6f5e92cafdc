"""Batch RL — host-side mirror of rl_coach/graph_managers/batch_rl_graph_manager.py (constructor :68-94, _create_graph
:96-154, improve :156-245).

A dataset is collected once — by random heat-up, or by a second, experience-generating agent that runs its own full
improve() under its own schedule on the same environment —, handed to the trained agent's memory, frozen and split into
training and evaluation episodes.  The trained agent never plays to learn: after the reward-model epochs
(improve_reward_model, which also builds DDQN-BCQ's key sets), the loop is "train the scheduled number of EPOCHS, then
evaluate against the environment".  Time is counted in epochs (TimeTypes.Epoch of the reference): the evaluation rows'
'Episode #' is the epoch, so a preset's max_episodes_to_achieve_reward bounds epochs.

Off-policy evaluation (:116,130,239,247-266) is switched by the attribute ``off_policy_evaluation`` (default False; set
it before create_graph): both agents' main wrappers get should_get_softmax_probabilities, so that the memories keep the
all_action_probabilities column; the evaluation set's static columns are gathered after improve_reward_model; after every
epoch's training and before the evaluation against the environment, run_off_policy_evaluation() computes IPS, DM, DR,
sequential DR and WIS (off_policy_evaluators/ope_manager.py), which go into that epoch's CSV row under the reference's
signal names.  With the switch off nothing of this exists and the CSV is what it was.

A dataset from a file (:97-104,141-154,174-177,234-241): when agent_params.memory.load_memory_from_file_path names a
core_types.CsvDataset, the trained agent's memory starts as that file (one device ingest launch, agents/dqn_agent.py
load_memory_from_file), and neither heat-up nor the experience-generating agent runs.  ``env_params=None`` together with
a ``spaces_definition`` (a vector observation and a DiscreteActionSpace) then runs without a simulator: the agent is
built on a stand-in (environments/dataset_environment.py) that cannot be stepped, every epoch's CSV row carries the
off-policy estimates and an empty 'Evaluation Reward'.  With ``checkpoint_save_dir`` set, a checkpoint of the trained
agent is saved after every epoch block (:234-236), named by the epoch.

Out of scope: NEC as the trained agent, pickled replay buffers, image observations and continuous actions in
files.
"""
from copy import deepcopy

from ..core_types import EnvironmentSteps, RunPhase
from .basic_rl_graph_manager import BasicRLGraphManager, dynamic_import


class BatchRLGraphManager(BasicRLGraphManager):
    def __init__(self, agent_params, env_params, schedule_params, vis_params=None, preset_validation_params=None,
                 name='batch_rl_graph', spaces_definition=None, reward_model_num_epochs=100, train_to_eval_ratio=0.8,
                 experience_generating_agent_params=None, experience_generating_schedule_params=None, device=None,
                 dist=None, csv_path=None):
        """Reference signature (:68-75) + where to run and where to log, as BasicRLGraphManager."""
        super().__init__(agent_params, env_params, schedule_params, vis_params, preset_validation_params, name,
                         device=device, dist=dist, csv_path=csv_path)
        self.is_batch_rl = True
        self.reward_model_num_epochs = reward_model_num_epochs
        self.spaces_definition = spaces_definition
        self.is_collecting_random_dataset = experience_generating_agent_params is None
        self.experience_generating_agent_params = experience_generating_agent_params
        self.experience_generating_schedule_params = experience_generating_schedule_params
        self.experience_generating_agent = None
        # by default the memory's ratio is 1 (no evaluation set), so it is set here (:84-89)
        if self.is_collecting_random_dataset:
            agent_params.memory.train_to_eval_ratio = train_to_eval_ratio
        else:
            experience_generating_agent_params.memory.train_to_eval_ratio = train_to_eval_ratio
        self.epochs = 0
        self.dataset_training_steps = 0     # updates of the experience-generating agent
        self.off_policy_evaluation = False  # set before create_graph: the five off-policy estimates after every epoch
        self.per_row_direct_method = False  # the paper's direct method instead of the reference's (ope_manager.py)
        self.ope_estimations = []           # one OpeEstimation per epoch
        self.checkpoint_save_dir = None     # a directory: a checkpoint of the trained agent after every epoch block

    def create_graph(self):                                                     # :96-154
        from ..agents.dqn_agent import DQNAgentParameters
        from ..compat import resolve_reference_style
        from ..memories.episodic.episodic_experience_replay import EpisodicExperienceReplayParameters
        from_file = getattr(self.agent_params.memory, "load_memory_from_file_path", None)
        if self.env_params is None:
            # (the reference only warns when there is neither, and then cannot train: :141-144)
            if not from_file:
                raise ValueError("A BatchRLGraph requires setting a dataset to load into the agent's memory or "
                                 "alternatively using an environment to create a (random) dataset from.")
            if self.spaces_definition is None:
                raise ValueError("a BatchRLGraphManager without an environment needs a spaces_definition")
        if not isinstance(self.agent_params, DQNAgentParameters):
            raise ValueError("Only DQN variants are supported at this point (NEC as the trained agent is not served)")
        if not isinstance(self.agent_params.memory, EpisodicExperienceReplayParameters):
            raise ValueError("Only Episodic memories are supported in Batch RL")
        rank = self.dist.rank if self.dist is not None else 0
        ap = self.agent_params
        if from_file and not self.is_collecting_random_dataset:
            # the file fills the TRAINED agent's memory, so the split ratio the constructor handed to the collecting
            # agent's memory belongs there (the reference leaves it at 1, and then has no evaluation set)
            ap.memory.train_to_eval_ratio = self.experience_generating_agent_params.memory.train_to_eval_ratio
        ap.is_batch_rl_training = True
        if 'reward_model' not in ap.network_wrappers:
            ap.network_wrappers['reward_model'] = deepcopy(ap.network_wrappers['main'])
        if self.off_policy_evaluation:                                          # :116,130
            ap.network_wrappers['main'].should_get_softmax_probabilities = True
            if not self.is_collecting_random_dataset:
                self.experience_generating_agent_params.network_wrappers['main'].should_get_softmax_probabilities = True
        resolve_reference_style(ap, self.env_params)
        env_params = self.env_params
        if env_params is None:
            from ..environments.dataset_environment import DatasetEnvironmentParameters
            env_params = DatasetEnvironmentParameters(self.spaces_definition)
        self.environment = dynamic_import(env_params.path)(env_params, self.device, rank=rank)
        self.trained_agent = dynamic_import(ap.path)(ap, self.environment, self.device, dist=self.dist,
                                                     use_graphs=self.use_graphs)
        if not self.is_collecting_random_dataset and self.env_params is not None:
            gp = self.experience_generating_agent_params
            gp.input_filter = getattr(ap, "input_filter", None)                 # :133-134
            resolve_reference_style(gp, self.env_params)
            self.experience_generating_agent = dynamic_import(gp.path)(gp, self.environment, self.device, dist=self.dist,
                                                                       use_graphs=self.use_graphs)
        self.agent = self.trained_agent
        return self

    def improve(self, should_stop=None):                                        # :156-245
        self.verify_graph_was_created()
        trained = self.trained_agent
        # with a dataset to load from, an environment is used for evaluating the policy only (:174-177)
        if getattr(trained.ap.memory, "load_memory_from_file_path", None):
            pass
        elif self.is_collecting_random_dataset:
            self.heatup(self.schedule.heatup_steps)
        else:
            # the experience-generating agent's full improve() under its own schedule, then its memory changes hands
            # (its episodes and evaluations are not logged: the reference turns its dump_csv off, :127)
            from .basic_rl_graph_manager import CsvLogger
            self.agent, own, log = self.experience_generating_agent, self.schedule, self.logger
            self.schedule = self.schedule_params = self.experience_generating_schedule_params
            self.logger = CsvLogger(None)
            super().improve()
            self.schedule = self.schedule_params = own
            self.agent, self.logger = trained, log
            self.dataset_training_steps, self.training_steps = self.training_steps, 0
            trained.memory = self.experience_generating_agent.memory
        trained.ap.algorithm.num_consecutive_playing_steps = EnvironmentSteps(0)      # this agent never actually plays
        trained.memory.drop_open_episode()
        trained.memory.freeze()
        trained.memory.prepare_evaluation_dataset()
        trained.improve_reward_model(self.reward_model_num_epochs)
        if self.off_policy_evaluation:                                          # :247-266
            from ..off_policy_evaluators.ope_manager import OpeManager
            trained.ope_manager = OpeManager(per_row_direct_method=self.per_row_direct_method)
            trained.ope_manager.gather_static_shared_stats(
                trained.memory, trained.ap.network_wrappers['reward_model'].batch_size, trained.networks['reward_model'])
        end = self.epochs + self.schedule.improve_steps.num_steps
        while self.epochs < end:
            self._set_phase(RunPhase.TRAIN)
            for _ in range(self.schedule.steps_between_evaluation_periods.num_steps):
                before = trained.training_iteration
                trained.train()
                self.training_steps += trained.training_iteration - before
                self.epochs += 1
            self._episodes_logged = self.epochs                                  # time is counted in epochs
            if self.checkpoint_save_dir is not None:                            # :234-236
                from ..checkpoint import save_checkpoint
                save_checkpoint(trained, self.checkpoint_save_dir, self.epochs)
            if self.off_policy_evaluation:                                      # :239
                self.ope_estimations.append(trained.run_off_policy_evaluation())
            if self.env_params is not None:                                     # :241
                self.evaluate(self.schedule.evaluation_steps)
            else:
                self.logger.write(**{"Episode #": self._episodes_logged, "Training Iter": trained.training_iteration,
                                     "Epoch": 0, "In Heatup": 0, "Total steps": trained.total_steps_counter},
                                  **self._evaluation_row_extras())
            if should_stop is not None and should_stop():
                break
        self.check_status()
        return self.logger.rows

    def run_preset_validation(self, *args, **kwargs):
        if self.env_params is None:
            raise ValueError("a preset's golden test needs evaluation rewards: this Batch RL graph has no environment")
        return super().run_preset_validation(*args, **kwargs)

    def _evaluation_row_extras(self):
        if not self.off_policy_evaluation or not self.ope_estimations:
            return {}
        from ..off_policy_evaluators.ope_manager import SIGNAL_NAMES
        return dict(zip(SIGNAL_NAMES, self.ope_estimations[-1]))
