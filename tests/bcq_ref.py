"""numpy restatement of the DDQN-BCQ pieces of Batch RL: the twin of csrc/bcq.hip and of the episodic replay's dataset
split, pinned to the reference's own code by tests/test_bcq_ref.py (recorded in tests/golden/bcq.npz).

  nn_min_distance(queries, keys, set_offsets) -> fp32 [n_queries, n_sets]
      what AnnoyDictionary._get_k_nearest_neighbors_indices(keys, 1) returns as distances (agents/ddqn_bcq_agent.py:109-111,
      :212-214), searched exactly.  Per (query, key) pair acc = 0; for w in order: t = fp32(q[w] - k[w]); acc = fp32(acc +
      fp32(t * t)); the set's value is sqrt (correctly rounded, fp32) of the minimum of acc over the set's keys; an empty
      set gives +inf.  The minimum is exact in any order, so a kernel may split the keys as it likes and still agree bit
      for bit.
  uniforms(B, A, seed, rank, event)              -> fp32 [B, A] in [0, 1): the top 24 bits of word 0 of Philox4x32-10 under
      the key (seed, rank) at the counter (event low word, event high word, b, a), times 2^-24.
  masked_selector(q, familiarity, threshold, ...) -> (sel, mask, zero_rows): DDQNBCQAgent.select_actions (:107-133) up to
      its argmax: -inf where fp64(familiarity) > threshold; a row whose maximum is then -inf takes the uniforms instead of
      the reference's np.random.rand (the number of such rows is device data: DESIGN §8).
  td_targets(...)                                 DQNAgent.learn_from_batch (agents/dqn_agent.py:92-103) with those actions
  reward_model_targets(prediction, actions, rewards)      value_optimization_agent.py:173-180
  average_dist(dist)                              ddqn_bcq_agent.py:212-216: per tree, per transition, summed in that order
  split(episode_lengths, ratio), shuffled_batches(n, size)   episodic_experience_replay.py:532-546, :179-184
"""
import math
import random

import numpy as np

from oracle.synth_env import philox4x32_10

F32 = np.float32


def squared_distances(queries, keys):
    """fp32 [n_queries, n_keys]: the pairs' accumulators after the whole width"""
    q = np.ascontiguousarray(queries, dtype=F32)
    k = np.ascontiguousarray(keys, dtype=F32).reshape(-1, q.shape[1])
    acc = np.zeros((q.shape[0], k.shape[0]), dtype=F32)
    for w in range(q.shape[1]):
        t = q[:, w, None] - k[None, :, w]
        acc = acc + t * t
    assert acc.dtype == F32
    return acc


def key_sets(embeddings, actions, n_actions):
    """ddqn_bcq_agent.py:202-207: action a's keys are the embeddings of the transitions with that action, in stored order
    -> (keys [n, W] grouped by action, set_offsets int32 [n_actions + 1])"""
    actions = np.asarray(actions)
    keys = np.concatenate([np.asarray(embeddings, dtype=F32)[actions == a] for a in range(n_actions)])
    counts = [int((actions == a).sum()) for a in range(n_actions)]
    return keys, np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def nn_min_distance(queries, keys, set_offsets):
    acc = squared_distances(queries, keys)
    out = np.full((acc.shape[0], len(set_offsets) - 1), np.inf, dtype=F32)
    for s in range(len(set_offsets) - 1):
        lo, hi = int(set_offsets[s]), int(set_offsets[s + 1])
        if hi > lo:
            out[:, s] = np.sqrt(acc[:, lo:hi].min(axis=1))
    return out


def uniforms(B, A, seed, rank, event):
    b, a = np.meshgrid(np.arange(B, dtype=np.uint64), np.arange(A, dtype=np.uint64), indexing="ij")
    ev = int(event) & 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(np.full_like(b, ev & 0xFFFFFFFF), np.full_like(b, ev >> 32), b, a, seed, rank)[0]
    return (w >> np.uint64(8)).astype(F32) * F32(5.9604644775390625e-8)


def masked_selector(q_next_online, familiarity, threshold, seed=0, rank=0, event=0):
    sel = np.array(q_next_online, dtype=F32)
    mask = np.asarray(familiarity).astype(np.float64) > float(threshold)
    sel[mask] = -np.inf
    zero_rows = sel.max(axis=1) == -np.inf
    if zero_rows.any():
        sel[zero_rows] = uniforms(sel.shape[0], sel.shape[1], seed, rank, event)[zero_rows]
    return sel, mask, zero_rows


def td_targets(q_online, q_next_target, selected_actions, actions, rewards, game_overs, discount):
    td = np.array(q_online, dtype=F32)
    for i in range(td.shape[0]):
        td[i, int(actions[i])] = np.float64(rewards[i]) + (1.0 - np.float64(bool(game_overs[i]))) * discount * \
            np.float64(q_next_target[i][int(selected_actions[i])])
    return td


def reward_model_targets(prediction, actions, rewards):
    t = np.array(prediction, dtype=F32)
    t[np.arange(t.shape[0]), np.asarray(actions, dtype=np.int64)] = np.asarray(rewards, dtype=F32)
    return t


def average_dist(dist):
    """dist [n_transitions, n_actions] (every transition against every action's set) -> the Python-order fp64 sum, tree
    by tree, divided by the number of transitions"""
    return sum([float(x) for s in range(dist.shape[1]) for x in dist[:, s]]) / dist.shape[0]


def split(episode_lengths, ratio):
    """-> (last_training_set_episode_id, last_training_set_transition_id)"""
    if ratio < 0 or ratio >= 1:
        raise ValueError('train_to_eval_ratio should be in the (0, 1] range.')
    n = sum(episode_lengths)
    index = round(ratio * n)
    if index >= n:
        raise IndexError('list index out of range')
    seen = 0
    for e, T in enumerate(episode_lengths):
        seen += T
        if index < seen:
            return e, seen


def shuffled_batches(n, size):
    """one random.shuffle on Python's stream over range(n), cut into ceil(n / size) batches"""
    idx = list(range(n))
    random.shuffle(idx)
    return [idx[i * size:(i + 1) * size] for i in range(math.ceil(n / size))]


class MLP64(object):
    """float64 restatement of a DQNNet on vector observations (embedder and middleware Dense + relu, a linear Q head) and
    of its whole layer-by-layer update: Double-DQN targets at given selected actions, the Q head's mean squared error
    over the batch, l2_regularization * sum(w^2) / 2 over EVERY weight (general_network.py:354-358), backward, TF1 Adam."""

    def __init__(self, named_arrays, lr, beta1=0.9, beta2=0.99, eps=1e-4):
        names = sorted({k.rsplit("/", 1)[0] for k in named_arrays if not k.endswith("q_head/dense/kernel")
                        and not k.endswith("q_head/dense/bias")}, key=lambda n: ("middleware" in n, n))
        names.append("main/q_head/dense")
        self.names = names
        self.W = [np.array(named_arrays[n + "/kernel"][0], dtype=np.float64) for n in names]
        self.b = [np.array(named_arrays[n + "/bias"][0], dtype=np.float64) for n in names]
        self.lr, self.b1, self.b2, self.eps, self.t = lr, beta1, beta2, eps, 0
        self.m = [np.zeros_like(x) for x in self.W + self.b]
        self.v = [np.zeros_like(x) for x in self.W + self.b]
        self.copy_to_target()

    def copy_to_target(self):
        self.target = ([w.copy() for w in self.W], [b.copy() for b in self.b])

    def forward(self, x, target=False, keep=False):
        W, b = self.target if target else (self.W, self.b)
        acts = [np.asarray(x, dtype=np.float64)]
        for i in range(len(W)):
            z = acts[-1] @ W[i] + b[i]
            acts.append(z if i == len(W) - 1 else np.maximum(z, 0.0))
        return acts if keep else acts[-1]

    def update(self, obs, nxt, actions, rewards, game_overs, discount, chosen, l2):
        """-> dict(loss, head_loss, norm): one update at the selected next actions `chosen`"""
        B = len(actions)
        rows = np.arange(B)
        q_next = self.forward(nxt, target=True)
        y = np.asarray(rewards, np.float64) + (1.0 - np.asarray(game_overs, np.float64)) * discount * q_next[rows, chosen]
        acts = self.forward(obs, keep=True)
        e = acts[-1][rows, actions] - y
        head_loss = float(np.mean(e * e))
        d = np.zeros_like(acts[-1])
        d[rows, actions] = 2.0 * e / B
        gW, gb = [None] * len(self.W), [None] * len(self.W)
        for i in reversed(range(len(self.W))):
            gW[i], gb[i] = acts[i].T @ d, d.sum(axis=0)
            if i:
                d = (d @ self.W[i].T) * (acts[i] > 0)
        sq = sum(float((w * w).sum()) for w in self.W + self.b)
        grads = [g + l2 * w for g, w in zip(gW + gb, self.W + self.b)]
        norm = float(np.sqrt(sum(float((g * g).sum()) for g in grads)))
        self.t += 1
        alpha = self.lr * np.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t)
        for k, (w, g) in enumerate(zip(self.W + self.b, grads)):
            self.m[k] += (g - self.m[k]) * (1.0 - self.b1)
            self.v[k] += (g * g - self.v[k]) * (1.0 - self.b2)
            w -= self.m[k] * alpha / (np.sqrt(self.v[k]) + self.eps)
        return dict(loss=head_loss + 0.5 * l2 * sq, head_loss=head_loss, norm=norm)
