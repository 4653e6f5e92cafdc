"""float64 restatement of csrc/returns.hip, one episode at a time: the twin of rlx_gae, rlx_discounted_returns,
rlx_standardize, rlx_episode_stats_step and rlx_episode_nstep_returns.  Written from the reference's formulas (paths
under rl_coach/): agents/actor_critic_agent.py:108-125, agents/clipped_ppo_agent.py:181-201, core_types.py:771-801,
agents/agent.py:558-601 -- NOT from oracle/returns.py, which this module never imports: tests/test_returns_ref.py compares
the two.

The scan kernels re-associate the recurrence; this module does not.  A trajectory is cut into episodes at game_over, every
episode is run on its own from 0.0, backwards, one step after the other (what scipy's lfilter does in the reference), and
only a trailing segment without a game_over sees the bootstrap.  So a non-finite reward or value stays inside its episode.

  split_episodes(game_over)                         -> [(start, stop, closed)]
  gae(rewards, values, game_over, bootstrap, discount, lam) -> (advantages, advantages + values), float64
  discounted_returns(rewards, game_over, discount)  -> float64
  standardize(x)                                    -> ((x - mean) / std, mean, std) with numpy's mean / std
  nstep_returns(rewards, discount, n_step)          -> core_types.py:771-801 with its pad-and-add order, float64
  EpisodeStats(n_env)                               -> per-env totals, last_return / last_len, the 8 accumulators

`python tests/returns_ref.py --against-reference` holds nstep_returns to the reference's own Episode class (needs the
reference tree; test_returns_ref.py runs it in a process of its own)."""
import numpy as np

F32 = np.float32
F64 = np.float64


def _f64(x):
    return np.asarray(x, dtype=F32).astype(F64)


def split_episodes(game_over):
    """[(start, stop, closed)]: steps [start, stop) form one episode; closed = its last step has game_over."""
    out, start = [], 0
    game_over = np.asarray(game_over)
    for t in range(len(game_over)):
        if game_over[t]:
            out.append((start, t + 1, True))
            start = t + 1
    if start < len(game_over):
        out.append((start, len(game_over), False))
    return out


def _discount_backwards(x, coef, tail):
    """y_t = x_t + coef * y_{t+1}, y_T = tail (lfilter([1], [1, -coef], x[::-1])[::-1] for tail = 0)"""
    y = np.empty(len(x), dtype=F64)
    acc = F64(tail)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(len(x) - 1, -1, -1):
            acc = x[t] + coef * acc
            y[t] = acc
    return y


def gae(rewards, values, game_over, bootstrap, discount, lam):
    """One sequence.  delta_t = r_t + discount * V_{t+1} - V_t (:118) with V past a game_over = 0 (clipped_ppo_agent.py:188)
    and V past an open end = bootstrap; A_t = delta_t + discount * lam * A_{t+1} (:119); value target = A + V (:121)."""
    r, v = _f64(rewards), _f64(values)
    boot = F64(F32(0.0 if bootstrap is None else bootstrap))
    adv = np.empty(len(r), dtype=F64)
    discount, lam = F64(discount), F64(lam)
    with np.errstate(invalid="ignore", over="ignore"):
        for a, b, closed in split_episodes(game_over):
            vnext = np.append(v[a + 1:b], 0.0 if closed else boot)
            adv[a:b] = _discount_backwards(r[a:b] + discount * vnext - v[a:b], discount * lam, 0.0)
        return adv, adv + v


def discounted_returns(rewards, game_over, discount):
    """One sequence.  R_t = r_t + discount * R_{t+1} inside an episode; an open last segment continues into 0."""
    r = _f64(rewards)
    out = np.empty(len(r), dtype=F64)
    for a, b, _ in split_episodes(game_over):
        out[a:b] = _discount_backwards(r[a:b], F64(discount), 0.0)
    return out


def standardize(x):
    """clipped_ppo_agent.py:201: (x - mean) / std, no epsilon"""
    x = np.asarray(x, dtype=F64)
    mean, std = np.mean(x), np.std(x)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (x - mean) / std, mean, std


def nstep_returns(rewards, discount, n_step):
    """Episode.update_discounted_rewards without the bootstrap branch: the reference's statements on a float64 copy."""
    if n_step != -1 and n_step < 1:
        raise ValueError("n-step should be an integer with value >= 1, or set to -1 for always setting to episode length.")
    rewards = _f64(rewards)
    length = len(rewards)
    curr_n_step = length if (n_step == -1 or n_step > length) else n_step
    discounted_rewards = rewards.copy()
    current_discount = F64(discount)
    for i in range(1, curr_n_step):
        discounted_rewards += current_discount * np.pad(rewards[i:], (0, i), 'constant', constant_values=0)
        current_discount *= discount
    return discounted_rewards


class EpisodeStats(object):
    """agent.py:558-601: total_reward_in_current_episode and current_episode_steps_counter per env, reset at game_over.
    last_return / last_len hold the totals of the env's most recent finished episode and keep what they held otherwise.
    acc = {episodes, sum R, sum R^2, max R, min R, sum len, max len, min len} over every finished episode; the sums are
    taken in float64 in one pass here, so they meet the device's tree sums to rounding only."""

    def __init__(self, n_env, last_return, last_len):
        self.ep_return = np.zeros(n_env, dtype=F64)
        self.ep_len = np.zeros(n_env, dtype=np.int32)
        self.last_return = np.array(last_return, dtype=F64)
        self.last_len = np.array(last_len, dtype=np.int32)
        self.returns, self.lengths = [], []

    def step(self, reward, done):
        done = np.asarray(done).astype(bool)
        self.ep_return = self.ep_return + _f64(reward)
        self.ep_len = self.ep_len + 1
        self.last_return[done] = self.ep_return[done]
        self.last_len[done] = self.ep_len[done]
        self.returns += self.ep_return[done].tolist()
        self.lengths += self.ep_len[done].tolist()
        self.ep_return[done] = 0.0
        self.ep_len[done] = 0

    def acc(self):
        r, l = np.array(self.returns, dtype=F64), np.array(self.lengths, dtype=F64)
        if len(r) == 0:
            return np.array([0, 0, 0, -np.inf, np.inf, 0, -np.inf, np.inf])
        return np.array([len(r), r.sum(), (r * r).sum(), r.max(), r.min(), l.sum(), l.max(), l.min()])


NSTEP_T = [1, 2, 255, 256, 257]


def nstep_cases(T):
    return [-1, 1, 2, 3, T - 1, T, T + 5]


def nstep_rewards(T):
    return np.random.RandomState(1000 + T).randn(T).astype(F32)


def _against_reference():
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import _refstub
    _refstub.install()
    from rl_coach.core_types import Episode, Transition
    checked = 0
    for T in NSTEP_T:
        rewards = nstep_rewards(T)
        for n_step in nstep_cases(T):
            if n_step == 0:
                continue
            ep = Episode(discount=0.97, n_step=n_step)
            for t in range(T):
                ep.insert(Transition(state={"observation": np.zeros(1)}, action=0, reward=float(rewards[t]),
                                     next_state={"observation": np.zeros(1)}, game_over=t == T - 1))
            ep.update_discounted_rewards()
            ref = np.array([tr.n_step_discounted_rewards for tr in ep.transitions], dtype=F64)
            mine = nstep_returns(rewards, 0.97, n_step)
            assert np.array_equal(ref.view(np.uint64), mine.view(np.uint64)), (T, n_step)
            checked += 1
    print("nstep_returns equals the reference's Episode in %d cases" % checked)


if __name__ == "__main__":
    import sys
    if "--against-reference" in sys.argv:
        _against_reference()
