"""numpy restatement of EpisodicHindsightExperienceReplay (rl_coach/memories/episodic/
episodic_hindsight_experience_replay.py:73-148 on top of episodic_experience_replay.py:210-317) on FLAT observation
vectors with a slice table — the form the device memory keeps (coach_amd/csrc/her.hip).

A finished episode of T transitions is walked in order (Future skips the last one); every walked transition gets k copies
appended to the SAME episode, transition ascending, copy ascending.  The goal of a copy is the `goal_name` slice of the
STATE of a selected transition: Final — the last one, no draw; Future — np.random.choice over transitions t+1 .. T-1;
Episode — np.random.choice over all T (one draw per copy on the global legacy stream, exactly where the reference
draws: np.random.choice(list of n) consumes what np.random.choice(n) consumes).  The copy's observation and next
observation carry the goal in the desired-goal slice; reward and game_over come from ReachingGoal on the fp64 distance,
summed in index order, between the goal and the `goal_name` slice of the copy's next observation.  The extended episode
enters the list as one episode; whole oldest episodes leave while the list holds more than max_size transitions.
tests/golden/her.npz holds what the reference's own class produced; this module must reproduce it exactly."""
import numpy as np

EUCLIDEAN, MANHATTAN = "Euclidean", "Manhattan"


def distance(goal, achieved, metric):
    """fp64, index order: sqrt(sum d^2) or sum |d|."""
    s = 0.0
    for g, a in zip(np.asarray(goal, dtype=np.float64).tolist(), np.asarray(achieved, dtype=np.float64).tolist()):
        d = g - a
        s = s + (d * d if metric == EUCLIDEAN else abs(d))
    return float(np.sqrt(np.float64(s))) if metric == EUCLIDEAN else s


def select_steps(method, T, k):
    """-> (n_base, int array [n_base * k]) the selected step of every copy, drawn in the reference's walk order."""
    n_base = T - 1 if method == "Future" else T
    sel = np.zeros(n_base * k, dtype=np.int32)
    for t in range(n_base):
        for j in range(k):
            if method == "Future":
                sel[t * k + j] = t + 1 + np.random.choice(T - t - 1)
            elif method == "Final":
                sel[t * k + j] = T - 1
            elif method == "Episode":
                sel[t * k + j] = np.random.choice(T)
            else:
                raise ValueError("supported goal selection methods: Final, Future, Episode")
    return n_base, sel


def relabel(obs, next_obs, actions, sel, n_base, k, goal_at, achieved_at, goal_dim, metric, threshold, reach_reward,
            default_reward):
    """the copies of one episode -> (obs, next_obs, actions, reward fp32, game_over uint8), n_base * k rows."""
    n = n_base * k
    o = np.repeat(obs[:n_base], k, axis=0).copy()
    no = np.repeat(next_obs[:n_base], k, axis=0).copy()
    a = np.repeat(actions[:n_base], k, axis=0).copy()
    r = np.zeros(n, dtype=np.float32)
    go = np.zeros(n, dtype=np.uint8)
    for c in range(n):
        goal = obs[sel[c], achieved_at:achieved_at + goal_dim]
        o[c, goal_at:goal_at + goal_dim] = goal
        no[c, goal_at:goal_at + goal_dim] = goal
        reached = distance(goal, next_obs[c // k, achieved_at:achieved_at + goal_dim], metric) <= threshold
        r[c] = reach_reward if reached else default_reward
        go[c] = 1 if reached else 0
    return o, no, a, r, go


class HindsightReplay(object):
    def __init__(self, max_size, k, method, goal_at, achieved_at, goal_dim, metric=EUCLIDEAN, threshold=0.0,
                 reach_reward=0.0, default_reward=-1.0):
        self.max_size, self.k, self.method = int(max_size), int(k), method
        self.goal_at, self.achieved_at, self.goal_dim = goal_at, achieved_at, goal_dim
        self.metric, self.threshold = metric, float(threshold)
        self.reach_reward, self.default_reward = reach_reward, default_reward
        self.episodes = []           # per complete episode: (obs, next_obs, actions, reward, game_over) arrays

    def store_episode(self, obs, next_obs, actions, rewards, game_overs):
        obs, next_obs = np.asarray(obs, dtype=np.float32), np.asarray(next_obs, dtype=np.float32)
        actions = np.asarray(actions)
        n_base, sel = select_steps(self.method, obs.shape[0], self.k)
        o, no, a, r, go = relabel(obs, next_obs, actions, sel, n_base, self.k, self.goal_at, self.achieved_at,
                                  self.goal_dim, self.metric, self.threshold, self.reach_reward, self.default_reward)
        self.episodes.append((np.concatenate([obs, o]), np.concatenate([next_obs, no]), np.concatenate([actions, a]),
                              np.concatenate([np.asarray(rewards, dtype=np.float32), r]),
                              np.concatenate([np.asarray(game_overs, dtype=np.uint8), go])))
        while self.max_size != 0 and self.num_transitions_in_complete_episodes() > self.max_size:
            self.episodes.pop(0)

    def num_transitions_in_complete_episodes(self):
        return sum(e[0].shape[0] for e in self.episodes)

    def num_complete_episodes(self):
        return len(self.episodes)

    def flat(self):
        """the reference's `transitions` list as columns."""
        keys = ("obs", "next_obs", "action", "reward", "game_over")
        return {k: np.concatenate([e[i] for e in self.episodes]) for i, k in enumerate(keys)}

    def sample_indices(self, size):
        if not self.episodes:
            raise ValueError("The episodic replay buffer cannot be sampled since there are no complete episodes yet.")
        return np.random.randint(self.num_transitions_in_complete_episodes(), size=size)
