"""numpy restatement of vanilla Policy Gradients' arithmetic (agents/policy_optimization_agent.py:72-135,
agents/policy_gradients_agent.py:98-133, core_types.py:780-801 and heads/policy_head.py:75-100 of the reference), the
twin of csrc/policy_gradient.hip.

The update window (fp64 throughout, ONE rounding to fp32 at the end):
  returns(rewards, discount)            -> fp64 [L]: Episode.update_discounted_rewards with n_step -1; rewards are the
                                           filtered rewards as the device keeps them (fp32), widened exactly
  Statistics(max_length)                   mean_return_over_multiple_episodes / num_episodes_where_step_has_been_seen
  window(rewards, start, discount, rescaler, stats) -> everything rlx_pg_episode_window computes; np.mean / np.std are
                                           numpy's own (pairwise summation)
  run(episodes, ...)                    -> the windows, counters and apply cadence of PolicyOptimizationAgent.train

The head (fp32 with the rounding points stated in head_rows; dtype=np.float64 evaluates the same formulas in fp64):
  head_rows(logits)                     -> p, q = p + eps, S = sum q, log pi = log q - log S, H = -sum (q / S) log pi
  head_loss(logits, actions, advantages, beta, T) -> loss, mean entropy, dlogits
  action_entropy(probs)                 -> -sum p log(p + eps) per row, fp32 (choose_action :154)
"""
import numpy as np

import c51_ref

F32 = np.float32
EPS = np.finfo(np.float32).eps                                       # rl_coach/utils.py: eps
TOTAL_RETURN, FUTURE_RETURN, FUTURE_RETURN_NORMALIZED_BY_EPISODE, FUTURE_RETURN_NORMALIZED_BY_TIMESTEP = range(4)
STATUS_EPISODE_TOO_LONG = 2


def returns(rewards, discount):
    """core_types.py:780-801 with n_step -1: current_discount * rewards[i:] added for i = 1 .. L-1, current_discount
    growing by repeated multiplication."""
    r = np.asarray(rewards, dtype=F32).astype(np.float64)
    out = r.copy()
    g = discount
    for i in range(1, r.size):
        out += g * np.pad(r[i:], (0, i), 'constant', constant_values=0)
        g *= discount
    return out


class Statistics(object):
    def __init__(self, max_length):
        self.mean = np.zeros(max_length)
        self.seen = np.zeros(max_length)


def window(rewards, start, discount, rescaler, stats):
    """One pass of PolicyOptimizationAgent.train's body over the episode so far (`rewards`, L entries) with the window
    episode[start:] -> dict, or None (status STATUS_EPISODE_TOO_LONG) when the episode is longer than the statistics
    arrays.  The statistics are updated over the WHOLE episode at every window, as the reference does."""
    L = len(rewards)
    if L > stats.mean.size:
        return None
    ret = returns(rewards, discount)
    ep_mean = ep_std = 0.0
    if rescaler in (FUTURE_RETURN_NORMALIZED_BY_EPISODE, FUTURE_RETURN_NORMALIZED_BY_TIMESTEP):
        for i in range(L):                                           # policy_optimization_agent.py:74-81
            stats.seen[i] += 1
            stats.mean[i] -= stats.mean[i] / stats.seen[i]
            stats.mean[i] += ret[i] / stats.seen[i]
        ep_mean, ep_std = np.mean(ret), np.std(ret)
    total = ret[start:].copy()
    for i in reversed(range(total.size)):                            # policy_gradients_agent.py:103-118
        if rescaler == TOTAL_RETURN:
            total[i] = total[0]
        elif rescaler == FUTURE_RETURN_NORMALIZED_BY_EPISODE:
            total[i] = (total[i] - ep_mean) / ep_std if ep_std != 0 else 0
        elif rescaler == FUTURE_RETURN_NORMALIZED_BY_TIMESTEP:
            total[i] -= stats.mean[i]                                # i: the position in the batch
    return dict(returns=ret, rescaled=total, advantages=total.astype(F32), returns_mean=np.mean(total),
                returns_std=np.std(total), episode_mean=ep_mean, episode_std=ep_std)


def run(episode_rewards, discount, rescaler, max_length, t_max=20000, apply_every=5, stats=None):
    """N consecutive episodes of one agent through PolicyOptimizationAgent.train, called after every step as the level
    manager does: the transition of a non-terminal step enters the episode buffer at the start of the NEXT step
    (level_manager.py:236-264), so train() sees one transition less than the steps taken until the terminal step, whose
    transition enters at once -> list of dict(episode, start, end, complete, current_episode, training_iteration,
    applied, + window)."""
    stats = Statistics(max_length) if stats is None else stats
    out, current_episode, training_iteration = [], 0, 0
    for e, rewards in enumerate(episode_rewards):
        last = 0
        for step in range(1, len(rewards) + 1):
            complete = step == len(rewards)
            if complete:
                current_episode += 1                                 # handle_episode_ended runs before train()
            visible = step if complete else step - 1
            if not (visible - last >= t_max or complete) or visible - last <= 0:
                continue
            w = window(rewards[:visible], last, discount, rescaler, stats)
            applied = current_episode % apply_every == 0
            training_iteration += 1
            out.append(dict(w, episode=e, start=last, end=visible, complete=complete, current_episode=current_episode,
                            training_iteration=training_iteration, applied=applied))
            last = 0 if complete else visible
    return out


def _seq_sum(x):
    s = np.zeros(x.shape[:-1], dtype=x.dtype)
    for j in range(x.shape[-1]):
        s = s + x[..., j]
    return s


def head_rows(logits, dtype=F32):
    """fp32: p = c51_ref.softmax (max, fp64 exp rounded once, fp32 sum in index order, fp32 division); q = p + eps (one
    fp32 addition); S = sum q in index order; log x = the fp64 log rounded to fp32 once; log pi = log q - log S (one fp32
    subtraction); H = -(sum in index order of (q / S) * log pi)."""
    if dtype is F32:
        p = c51_ref.softmax(logits)
        log = lambda v: np.log(v.astype(np.float64)).astype(F32)
    else:
        p = c51_ref.softmax_f64(logits)
        log = np.log
    q = p + dtype(EPS)
    S = _seq_sum(q)
    lp = log(q) - log(S)[..., None]
    H = -_seq_sum((q / S[..., None]) * lp)
    return p, q, S, lp, H


def head_loss(logits, actions, advantages, beta, T=None, dtype=F32):
    """logits [R, A]; rows [T, R) are padding.  loss = -(1/T) sum_b log pi_b(a_b) adv_b - beta (1/T) sum_b H_b.
    dlogits through dlog pi_a/dp_k = [k == a]/q_a - 1/S, dH/dp_k = -(log pi_k + H)/S, dz_j = p_j (g_j - sum_k g_k p_k).
    A row whose action is outside [0, A) has no term and a zero gradient (status bit 0)."""
    x = np.asarray(logits, dtype=dtype)
    R, A = x.shape
    T = R if T is None else T
    act = np.asarray(actions)[:T]
    adv = np.asarray(advantages, dtype=dtype)[:T]
    valid = (act >= 0) & (act < A)
    p, q, S, lp, H = head_rows(x[:T], dtype)
    a = np.where(valid, act, 0)
    rows = np.arange(T)
    fT, b = dtype(T), dtype(beta)
    pol = (lp[rows, a] * adv)[valid].sum(dtype=dtype)
    ent = H[valid].sum(dtype=dtype)
    mean_h = ent / fT
    loss = -(pol / fT) - b * mean_h
    onehot = np.zeros((T, A), dtype=dtype)
    onehot[rows, a] = 1
    dlog = onehot * (dtype(1) / q) - (dtype(1) / S)[:, None]
    g = (b / fT) * ((lp + H[:, None]) / S[:, None]) - (adv / fT)[:, None] * dlog
    dot = _seq_sum(g * p)
    d = np.zeros((R, A), dtype=dtype)
    d[:T] = np.where(valid[:, None], p * (g - dot[:, None]), 0)
    return dict(loss=loss, entropy=mean_h, dlogits=d, status=int(not valid.all()))


def action_entropy(probs):
    p = np.asarray(probs, dtype=F32)
    return -_seq_sum(p * np.log((p + F32(EPS)).astype(np.float64)).astype(F32))
