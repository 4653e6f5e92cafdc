"""numpy restatement of Rainbow DQN's arithmetic, the twin of csrc/rainbow.hip and csrc/nstep_store.hip: the reference's
agents/rainbow_dqn_agent.py:88-137, heads/rainbow_q_head.py:43-70, core_types.py:771-820 and the store loop of
agents/agent.py:571-574, operation by operation.  Reuses c51_ref for everything a categorical head does with logits.

v [.., N] fp32 (state-value stream), x [.., A, N] fp32 (action-advantage stream), z [N] fp64.
  merge(v, x)                          -> fp32 [.., A, N]: rlx_dueling_combine's order per atom (the sum starts at 0.f and
                                          takes the actions ascending; TensorFlow's own reduce_mean order is not pinned)
  merge_backward(dy)                   -> (dv [.., N], dx [.., A, N]): rlx_dueling_combine_backward's arithmetic per atom
  project(p_sel, p_tgt, z, R, boot, discount_n, ...)
                                       -> (a* [B], m [B, N] fp32): rainbow_dqn_agent.py:91-119 — a* on the ONLINE
                                          network's distributions on s', the TARGET network's distribution projected
  update(...)                          -> everything rlx_rainbow_head_loss computes
  process_episode(T, rewards, n, g)    -> (next-state index [T], bootstrap flags [T], n-step returns [T] fp64)
  EpisodeStore                         -> the host loop of the memory: per-env staging, episodes stored when they end, in
                                          env order, into a ring
"""
import numpy as np

import c51_ref

F32 = np.float32


def merge(v, x):
    v, x = np.asarray(v, dtype=F32), np.asarray(x, dtype=F32)
    A = x.shape[-2]
    s = np.zeros(x.shape[:-2] + x.shape[-1:], dtype=F32)
    for a in range(A):
        s = s + x[..., a, :]
    mean = s / F32(A)
    return (v[..., None, :] + (x - mean[..., None, :])).astype(F32)


def merge_backward(dy):
    dy = np.asarray(dy, dtype=F32)
    A = dy.shape[-2]
    s = np.zeros(dy.shape[:-2] + dy.shape[-1:], dtype=F32)
    for a in range(A):
        s = s + dy[..., a, :]
    mean = s / F32(A)
    return s, (dy - mean[..., None, :]).astype(F32)


def project(p_select, p_target, z, returns, bootstrap, discount_n, device_order=False, overhang="raise"):
    """rainbow_dqn_agent.py:91-119.  p_select: the online network's distributions on s' (the Double-DQN choice),
    p_target: the target network's; returns fp64 [B] (n_step_discounted_rewards), bootstrap [B]
    (should_bootstrap_next_state), discount_n = discount ** n_step.  overhang: see c51_ref.project."""
    B = p_target.shape[0]
    q = c51_ref.q_values_device_order(p_select, z) if device_order else c51_ref.q_values(p_select, z)
    a_star = np.argmax(q, axis=1)
    R = np.asarray(returns, dtype=np.float64)
    boot = np.asarray(bootstrap).astype(bool)
    m = np.zeros((B, z.size))
    rows = np.arange(B)
    for j in range(z.size):
        tzj = np.fmax(np.fmin(R + boot * discount_n * z[j], z[-1]), z[0])
        bj = (tzj - z[0]) / (z[1] - z[0])
        u = (np.ceil(bj)).astype(int)
        l = (np.floor(bj)).astype(int)
        m[rows, l] += (p_target[rows, a_star, j] * (u - bj))
        ok = u < z.size if overhang == "drop" else slice(None)
        m[rows[ok], u[ok]] += (p_target[rows, a_star, j] * (bj - l))[ok]
    return a_star, m.astype(F32)


def update(v, x, v_next_target, x_next_target, v_next_online, x_next_online, z, actions, returns, bootstrap, discount_n,
           grad_scale=1.0, dtype=F32, overhang="raise"):
    """-> dict(merged, a_star, m, action_losses [B, A], loss, dlogits [B, A, N], dv [B, N], dx [B, A, N], errors [B]
    fp64): everything rlx_rainbow_head_loss computes (valid actions).  dtype=np.float64 evaluates the softmax-dependent
    values in fp64 from the same merged logits, a* and m."""
    y = merge(v, x)
    a_star, m = project(c51_ref.softmax(merge(v_next_online, x_next_online)),
                        c51_ref.softmax(merge(v_next_target, x_next_target)), z, returns, bootstrap, discount_n,
                        device_order=True, overhang=overhang)
    ce, loss, d = c51_ref.loss_and_grad(y, m, actions, dtype)
    d = (dtype(grad_scale) * d).astype(dtype)
    dv, dx = merge_backward(d) if dtype is F32 else (d.sum(axis=-2), d - d.mean(axis=-2, keepdims=True))
    return dict(merged=y, a_star=a_star, m=m, action_losses=ce, loss=loss, dlogits=d, dv=dv, dx=dx,
                errors=ce[np.arange(y.shape[0]), actions].astype(np.float64))


def nstep_returns(rewards, n_step, discount):
    """Episode.update_discounted_rewards (core_types.py:780-792) without the bootstrap from the old policy."""
    T = len(rewards)
    n = T if (n_step == -1 or n_step > T) else n_step
    r = np.array(rewards).astype('float')
    out = r.copy()
    g = discount
    for i in range(1, n):
        out += g * np.pad(r[i:], (0, i), 'constant', constant_values=0)
        g *= discount
    return out


def process_episode(rewards, n_step, discount):
    """Episode.update_transitions_rewards_and_bootstrap_data (core_types.py:803-820) for an episode of T = len(rewards)
    transitions -> (nxt [T], boot [T] bool, returns [T] fp64): transition k's next state is the STATE of transition nxt[k]
    where boot[k], and the NEXT state of transition T - 1 (nxt[k] == T) where not."""
    T = len(rewards)
    if n_step < 2:
        raise ValueError("the n-step redirection needs n_step >= 2 (the reference sets no bootstrap flag otherwise)")
    c = n_step if n_step < T else T
    nxt = np.array([k + c if k + c < T else T for k in range(T)], dtype=np.int64)
    return nxt, nxt < T, nstep_returns(rewards, n_step, discount)


class HostPriorities(object):
    """The leaves of PrioritizedExperienceReplay's three trees as flat host arrays (prioritized_experience_replay.py
    :188-201, :264-283): a stored transition takes maximal_priority; an update writes (error + epsilon) leaf by leaf and
    re-reads maximal_priority from the max tree — the maximum over the leaves as they are NOW, which may go down."""

    def __init__(self, capacity, alpha, epsilon):
        self.cap, self.alpha, self.epsilon = capacity, alpha, epsilon
        self.leaves = np.zeros(capacity)              # priority ** alpha (sum / min trees)
        self.priority = np.zeros(capacity)            # priority (max tree)
        self.max_p, self.stored, self.listed = 1.0, 0, 0

    def store(self, n=1):
        for _ in range(n):
            leaf = self.stored % self.cap
            self.leaves[leaf], self.priority[leaf] = self.max_p ** self.alpha, self.max_p
            self.stored += 1
            self.listed = min(self.listed + 2, self.cap)          # the doubled num_transitions()

    def update(self, idx, errors):
        for leaf, err in zip(idx, errors):
            p = float(err) + self.epsilon
            self.leaves[leaf], self.priority[leaf] = p ** self.alpha, p
            self.max_p = float(self.priority.max())


class EpisodeStore(object):
    """The host loop of the n-step prioritized memory: per-env staging; an env's episode is processed and appended when
    it ends, envs in order within a step; an open episode can be dropped.  Rows are dicts of host values; `ring` holds
    the `rows` most recent positions like the device ring (store number g lives at g % rows)."""

    def __init__(self, n_env, rows, n_step, discount):
        self.n_env, self.rows, self.n_step, self.discount = n_env, rows, n_step, discount
        self.staged = [[] for _ in range(n_env)]
        self.ring = [None] * rows
        self.stored = 0

    def step(self, obs, actions, rewards, game_overs, next_obs, dones):
        """one vector step -> the number of transitions that became visible."""
        n = 0
        for e in range(self.n_env):
            self.staged[e].append(dict(obs=np.array(obs[e], dtype=F32), action=int(actions[e]),
                                       reward=F32(rewards[e]), game_over=int(game_overs[e]),
                                       next_obs=np.array(next_obs[e], dtype=F32)))
        for e in range(self.n_env):
            if dones[e]:
                n += self._flush(e)
        return n

    def drop(self, env=None):
        for e in (range(self.n_env) if env is None else [env]):
            self.staged[e] = []

    def _flush(self, e):
        ep, self.staged[e] = self.staged[e], []
        nxt, boot, ret = process_episode([t["reward"] for t in ep], self.n_step, self.discount)
        for k, t in enumerate(ep):
            row = dict(obs=t["obs"], action=t["action"], reward=t["reward"], game_over=t["game_over"],
                       next_obs=ep[nxt[k]]["obs"] if boot[k] else ep[-1]["next_obs"],
                       n_step_discounted_rewards=ret[k], should_bootstrap_next_state=int(boot[k]))
            self.ring[self.stored % self.rows] = row
            self.stored += 1
        return len(ep)

    def column(self, key, rows):
        return np.array([self.ring[r][key] for r in rows])
