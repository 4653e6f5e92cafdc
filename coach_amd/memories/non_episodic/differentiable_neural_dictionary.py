"""Neural Episodic Control's dictionary on one MI355X — device mirror of QDND / AnnoyDictionary
(rl_coach/memories/non_episodic/differentiable_neural_dictionary.py:29-268) and of the arithmetic of DNDQHead
(architectures/tensorflow_components/heads/dnd_q_head.py:67-83).  Pritzel et al. 2017.

One table per action, all on the device: keys [A, cap, W], values [A, cap], LRU stamps [A, cap] (int64), sizes [A] and
one clock.  Nothing here computes: every method is launches of csrc/dnd.hip (rlx_dnd_lookup, rlx_dnd_head_forward,
rlx_dnd_head_loss_backward, rlx_dnd_add), no table ever travels to the host, and no method synchronises except
`has_enough_entries`, which reads the A sizes.

Deviations from the reference, on purpose:
  * the search is exact and ordered by (distance, index), where the Annoy forest is approximate;
  * a write is visible to the next lookup (the reference's index sees it after its next rebuild: the contract here is
    rebuild_on_every_update=True);
  * within one `add` the keys are looked up against the tables as they were before the call, every entry matched by a
    key of the call is stamped before the oldest entries are chosen, and the evicted set is the m oldest
    (stamp, index) pairs;
  * `train_query` looks up and stamps only the taken action's table: the other columns of the loss have zero gradient.
Not served, refused by name: propagate_updates_to_DND (ordered scatter-adds into the tables), checkpointing the tables.
"""
import ctypes

import torch

from ..._rlx import current_stream, lib

MAX_WIDTH, MAX_K = 512, 64


class QDND(object):
    def __init__(self, dict_size, key_width, num_actions, new_value_shift_coefficient=0.1, key_error_threshold=0.01,
                 num_neighbors=50, l2_norm_added_delta=0.001, propagate_updates_to_DND=False, device="cuda"):
        if propagate_updates_to_DND:
            raise NotImplementedError("QDND: propagate_updates_to_DND=True is not served (ordered scatter-adds into the "
                                      "tables; no preset sets it)")
        if key_width % 16 or not 16 <= key_width <= MAX_WIDTH:
            raise ValueError("QDND: key_width {} is not a multiple of 16 in [16, {}]".format(key_width, MAX_WIDTH))
        if not 1 <= num_neighbors <= MAX_K:
            raise ValueError("QDND: num_neighbors {} outside [1, {}]".format(num_neighbors, MAX_K))
        if not 1 <= dict_size <= 1 << 22:
            raise ValueError("QDND: dict_size {} outside [1, 2^22]".format(dict_size))
        if num_actions < 1:
            raise ValueError("QDND: num_actions {} below 1".format(num_actions))
        self.cap, self.W, self.A, self.k = int(dict_size), int(key_width), int(num_actions), int(num_neighbors)
        self.shift, self.threshold = float(new_value_shift_coefficient), float(key_error_threshold)
        self.delta = float(l2_norm_added_delta)
        self.lib, self.dev = lib(), device
        A, cap, W = self.A, self.cap, self.W
        self.keys = torch.zeros(A, cap, W, dtype=torch.float32, device=device)
        self.values = torch.zeros(A, cap, dtype=torch.float32, device=device)
        self.stamps = torch.zeros(A, cap, dtype=torch.int64, device=device)
        self.size = torch.zeros(A, dtype=torch.int32, device=device)
        self.clock = torch.zeros(1, dtype=torch.int64, device=device)
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.max_keys = 0          # the host's upper bound of every size: the number of chunks a lookup launches
        self._bufs = {}

    # ---------------------------------------------------------------------------------------------------- buffers
    def _buf(self, name, shape, dtype):
        t = self._bufs.get(name)
        if t is None or t.shape != torch.Size(shape) or t.dtype != dtype:
            t = self._bufs[name] = torch.zeros(shape, dtype=dtype, device=self.dev)
        return t

    def _scratch(self, rows, n_lists, k):
        nbytes = ctypes.c_longlong()
        self.lib.dnd_lookup_scratch_bytes(rows, n_lists, max(1, self.max_keys), k, ctypes.byref(nbytes))
        t = self._bufs.get("scratch")
        if t is None or t.numel() * 8 < nbytes.value:
            t = self._bufs["scratch"] = torch.zeros(max(1, nbytes.value // 8), dtype=torch.int64, device=self.dev)
        return t, nbytes.value

    @staticmethod
    def _rows(x, what):
        if x.dim() != 2 or x.dtype != torch.float32 or x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16:
            raise ValueError("QDND: {} must be fp32 [rows, W], 16-byte aligned rows with a stride that is a multiple of 4"
                             .format(what))
        return x

    def _vector(self, x, n, dtype, what):
        """a per-row argument as the kernels read it: contiguous [n] of `dtype` on the dictionary's device"""
        if not torch.is_tensor(x) or x.dtype != dtype or tuple(x.shape) != (n,) or not x.is_contiguous() or \
                x.device != self.keys.device:
            raise ValueError("QDND: {} must be a contiguous {} [{}] tensor on {}".format(what, dtype, n, self.keys.device))
        return x

    # ---------------------------------------------------------------------------------------------------- lookup
    def lookup(self, queries, actions=None, k=None, min_keys=None, with_dist=False, tag="lookup"):
        """(idx int32 [Q, A or 1, k], dist2 or None, flags int32 [Q, A or 1]).  actions None: every table; an int32 [Q]
        tensor: each query's own table."""
        q = self._rows(queries, "queries")
        k = self.k if k is None else int(k)
        n, n_lists = q.shape[0], self.A if actions is None else 1
        if actions is not None:
            self._vector(actions, n, torch.int32, "actions")
        idx = self._buf(tag + "_idx", (n, n_lists, k), torch.int32)
        dist = self._buf(tag + "_dist", (n, n_lists, k), torch.float32) if with_dist else None
        flags = self._buf(tag + "_flags", (n, n_lists), torch.int32)
        scratch, nbytes = self._scratch(n, n_lists, k)
        self.lib.dnd_lookup(q, q.stride(0), n, self.W, self.keys, self.W, self.cap, self.size, self.A,
                            max(1, self.max_keys), actions, n_lists, k, k + 1 if min_keys is None else int(min_keys),
                            idx, dist, flags, scratch, nbytes, current_stream())
        return idx, dist, flags

    # ---------------------------------------------------------------------------------------------------- the head
    def _head(self, embedding, actions, tag):
        e = self._rows(embedding, "embedding")
        idx, _, flags = self.lookup(e, actions, tag=tag)
        n, n_lists = idx.shape[0], idx.shape[1]
        q = self._buf(tag + "_q", (n, n_lists), torch.float32)
        d = self._buf(tag + "_d", (n, n_lists, self.k), torch.float32)
        sumw = self._buf(tag + "_sumw", (n, n_lists), torch.float32)
        self.lib.dnd_head_forward(e, e.stride(0), n, self.W, self.keys, self.W, self.cap, self.values, self.stamps, self.A,
                                  idx, flags, actions, n_lists, self.k, self.delta, self.clock, q, n_lists, d, sumw,
                                  current_stream())
        return q, (idx, flags, d, sumw)

    def query(self, embedding):
        """the acting pass: Q [rows, A] over all tables (zeros where a table has at most k entries); stamps what it read"""
        return self._head(embedding, None, "act")[0]

    def train_query(self, embedding, actions):
        """the training pass: Q [rows, 1] of each row's taken action, and what `loss_backward` needs"""
        return self._head(embedding, actions, "train")

    def loss_backward(self, embedding, actions, q, saved, targets, grad_scale=1.0, out=None):
        """(dE [rows, W], scalars [1] = the Q head's loss) of train_query's output against `targets` [rows]; out: the
        buffer that receives dE (a network's gradient of its trunk output)"""
        e = self._rows(embedding, "embedding")
        idx, flags, d, sumw = saved
        n = e.shape[0]
        self._vector(actions, n, torch.int32, "actions")
        self._vector(targets, n, torch.float32, "targets")
        de = self._buf("train_de", (n, self.W), torch.float32) if out is None else self._rows(out, "out")
        scalars = self._buf("train_scalars", (1,), torch.float32)
        self.lib.dnd_head_loss_backward(e, e.stride(0), n, self.W, self.keys, self.W, self.cap, self.values, self.A, idx,
                                        flags, actions, self.k, d, sumw, q, q.stride(0), targets, float(grad_scale), de,
                                        de.stride(0), scalars, current_stream())
        return de, scalars

    # ---------------------------------------------------------------------------------------------------- writes
    def add(self, embeddings, actions, values):
        """the episode-end write: T embeddings, their actions (int32) and returns (fp32), in episode order.  max_keys
        advances by T whatever the launch does with the rows (a call it drops because the clock reached 2^40, a row whose
        action names no table): it is only an upper bound of the sizes, which fixes the number of chunks a lookup
        launches; the sizes themselves are read on the device, so results stay correct."""
        e = self._rows(embeddings, "embeddings")
        T = e.shape[0]
        if T > self.cap:
            raise ValueError("QDND.add: {} keys exceed dict_size {}".format(T, self.cap))
        self._vector(values, T, torch.float32, "values")
        idx, dist, flags = self.lookup(e, actions, k=1, min_keys=1, with_dist=True, tag="add")
        slots = self._buf("add_slots", ((self.A + 1) * T,), torch.int32)
        self.lib.dnd_add(e, e.stride(0), T, self.W, actions, values, idx, dist, flags, self.keys, self.W, self.cap,
                         self.values, self.stamps, self.size, self.A, self.clock, self.threshold, self.shift, slots,
                         self.status, current_stream())
        self.max_keys = min(self.cap, self.max_keys + T)
        return True

    def has_enough_entries(self, k=None):
        """every table holds more than k entries (reads the A sizes: the one synchronising method)"""
        return bool((self.size > (self.k if k is None else int(k))).all().item())

    def check_status(self):
        s = int(self.status.item())
        if s:
            self.status.zero_()
            raise ValueError("QDND.add reported invalid input (status %d: 1 = an action outside [0, %d), 2 = the clock "
                             "passed 2^40)" % (s, self.A))
