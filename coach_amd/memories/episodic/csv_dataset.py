"""A logged dataset becomes flat tables — the host half of EpisodicExperienceReplay.load_csv
(rl_coach/memories/episodic/episodic_experience_replay.py:440-495), numpy and the standard library only.

The reference reads the file with pandas and builds one Transition object per row (DataFrame.iterrows), episode by
episode.  Here the file is parsed ONCE into flat arrays — features fp64 [R, D], action int32 [R], reward fp64 [R],
probabilities fp32 [R, A] — plus, per surviving transition t, the file rows it is made of: src[t] (state, action, reward,
probabilities), src_next[t] (next state) and last[t] (the episode's last transition).  The device half
(rlx_dataset_ingest, csrc/dataset.hip) turns them into replay rows with one launch.

The schema is the reference's: `episode_id`, `action`, `reward`, every column whose name starts with `state_feature` (in
header order) and `all_action_probabilities` (a quoted Python list, ast.literal_eval); other columns — transition_number,
episode_name ... — are ignored.  Episodes are taken in the order their id first appears (df['episode_id'].unique()); an
episode's rows are ALL rows of that id in file order, contiguous or not; an episode of T rows gives T - 1 transitions (one
of fewer than 2 rows gives none and is skipped); whole oldest episodes leave while the memory would hold more than
max_size (_enforce_max_length :210-222, run after every store_episode — what survives is the longest suffix that fits).

Departures: numbers are parsed with Python's correctly rounded float(), the reference's pandas uses its fast parser, and
the two can differ in the last place of a double (everything that reaches the device is fp32, as the acting path stores
it); all_action_probabilities is required only where the memory keeps that column (the reference always reads it); a bad
cell is a ValueError that names the file row.
"""
import ast
import csv
import re
import warnings

import numpy as np

from ..memory import MemoryGranularity

EPISODE_ID, ACTION, REWARD, PROBABILITIES = 'episode_id', 'action', 'reward', 'all_action_probabilities'
STATE_PREFIX = 'state_feature'
_PLAIN_LIST = re.compile(r"\[[0-9eE+\-., ]*\]")


class CsvTables(object):
    """What read_csv_dataset returns.  R file rows, N surviving transitions:
    features fp64 [R, D], action int32 [R], reward fp64 [R], probabilities fp32 [R, A] or None;
    src, src_next int32 [N], last uint8 [N]; episode_lengths: transitions of every surviving episode, oldest first;
    all_episode_lengths: the same before the capacity rule."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def n_file_rows(self):
        return self.features.shape[0]

    @property
    def n_transitions(self):
        return self.src.shape[0]


def _where(i):
    """how a message names data row i (0-based, as the reference's DataFrame index): the header is line 1"""
    return "file row %d (line %d)" % (i, i + 2)


def _floats(cells, what, path):
    """one column of texts -> fp64, correctly rounded (float()); a bad cell is a ValueError naming its row"""
    try:
        return np.array([float(c) for c in cells], dtype=np.float64)
    except ValueError:
        for i, c in enumerate(cells):
            try:
                float(c)
            except ValueError:
                raise ValueError("%s: %s of %s is not a number: %r" % (path, what, _where(i), c)) from None
        raise


def surviving_episodes(lengths, max_size):
    """_enforce_max_length (:210-222) after every store_episode -> index of the first episode that survives.
    lengths: transitions per stored episode, in order; max_size: (MemoryGranularity, n)."""
    granularity, size = max_size
    first, held = 0, 0
    for k, T in enumerate(lengths):
        held += T
        if granularity == MemoryGranularity.Transitions:
            while size != 0 and held > size:
                held -= lengths[first]
                first += 1
        else:
            while k + 1 - first > size:
                held -= lengths[first]
                first += 1
    return first


def _probabilities(cells, n_actions, path):
    out = np.empty((len(cells), n_actions), dtype=np.float32)
    for i, c in enumerate(cells):
        s = c.strip()
        try:
            if _PLAIN_LIST.fullmatch(s):            # a plain list of numbers: what ast.literal_eval would make of it
                body = s[1:-1].strip()
                p = [float(x) for x in body.split(',')] if body else []
            else:
                p = ast.literal_eval(s)
                if not isinstance(p, (list, tuple)):
                    raise ValueError("not a list")
                p = [float(x) for x in p]
        except (ValueError, SyntaxError, TypeError):
            raise ValueError("%s: %s of %s is not a list of numbers: %r" % (path, PROBABILITIES, _where(i), c)) from None
        if len(p) != n_actions:
            raise ValueError("%s: %s of %s has %d entries, the action space has %d actions"
                             % (path, PROBABILITIES, _where(i), len(p), n_actions))
        out[i] = p
    return out


def check_header(path, want_probabilities):
    """the file's first line alone: are the required columns there? (cheap: an agent asks before it builds anything)"""
    with open(path, newline='') as f:
        try:
            header = [h.strip() for h in next(csv.reader(f))]
        except StopIteration:
            raise ValueError("%s: the file is empty" % path) from None
    for name in [EPISODE_ID, ACTION, REWARD] + ([PROBABILITIES] if want_probabilities else []):
        if name not in header:
            raise ValueError("%s: the column %r is missing (the file has: %s)" % (path, name, ", ".join(header)))
    if not any(name.startswith(STATE_PREFIX) for name in header):
        raise ValueError("%s: no column starts with %r" % (path, STATE_PREFIX))
    return header


def read_csv_dataset(path, n_actions, want_probabilities, observation_dim=None, max_size=None):
    """-> CsvTables.  n_actions: A of the action space; want_probabilities: does the memory keep the
    all_action_probabilities column (then the file must have it; otherwise the file's column is ignored);
    observation_dim: D of the observation space (None: whatever the file has); max_size: the memory's
    (MemoryGranularity, n) — None keeps every episode."""
    with open(path, newline='') as f:
        reader = csv.reader(f)
        try:
            header = [h.strip() for h in next(reader)]
        except StopIteration:
            raise ValueError("%s: the file is empty" % path) from None
        rows = [r for r in reader if r]
    col = {}
    for j, name in enumerate(header):
        col.setdefault(name, j)
    state_cols = [j for j, name in enumerate(header) if name.startswith(STATE_PREFIX)]
    needed = [EPISODE_ID, ACTION, REWARD] + ([PROBABILITIES] if want_probabilities else [])
    for name in needed:
        if name not in col:
            raise ValueError("%s: the column %r is missing (the file has: %s)" % (path, name, ", ".join(header)))
    D = len(state_cols)
    if D == 0:
        raise ValueError("%s: no column starts with %r" % (path, STATE_PREFIX))
    if observation_dim is not None and D != int(observation_dim):
        raise ValueError("%s: the header (line 1) has %d %s columns, the observation space has %d features"
                         % (path, D, STATE_PREFIX, int(observation_dim)))
    R, width = len(rows), len(header)
    for i, r in enumerate(rows):
        if len(r) != width:
            raise ValueError("%s: %s has %d cells, the header has %d (%d %s columns are expected)"
                             % (path, _where(i), len(r), width, D, STATE_PREFIX))
    features = np.empty((R, D), dtype=np.float64)
    for k, j in enumerate(state_cols):
        features[:, k] = _floats([r[j] for r in rows], header[j], path)
    reward = _floats([r[col[REWARD]] for r in rows], REWARD, path)
    # int(row['action']) of the reference: a number, truncated; NaN or text is refused
    j = col[ACTION]
    action = np.empty(R, dtype=np.int32)
    for i, r in enumerate(rows):
        try:
            a = int(float(r[j]))
        except (ValueError, OverflowError):
            raise ValueError("%s: action of %s is not a number: %r" % (path, _where(i), r[j])) from None
        action[i] = a if -2 ** 31 <= a < 2 ** 31 else -1          # (outside every action space either way)
    probabilities = _probabilities([r[col[PROBABILITIES]] for r in rows], int(n_actions), path) \
        if want_probabilities else None
    if max_size is not None and R > max_size[1]:
        warnings.warn("Warning! The number of transitions to load into the replay buffer ({}) is "
                      "bigger than the max size of the replay buffer ({}). The excessive transitions will "
                      "not be stored.".format(R, max_size[1]))
    # episodes in order of first appearance; a numeric id column compares as numbers, as pandas would parse it
    ids = [r[col[EPISODE_ID]].strip() for r in rows]
    try:
        keys = np.array([float(x) for x in ids], dtype=np.float64)
        usable = ~np.isnan(keys)                                   # (df['episode_id'] == nan selects nothing)
    except ValueError:
        keys, usable = np.array(ids), np.ones(R, dtype=bool)
    episodes = []
    if R:
        _, first_index, inverse = np.unique(keys, return_index=True, return_inverse=True)
        inverse = inverse.reshape(-1)
        by_group = np.argsort(inverse, kind='stable')              # file order inside a group
        bounds = np.concatenate([[0], np.cumsum(np.bincount(inverse, minlength=len(first_index)))])
        for g in np.argsort(first_index, kind='stable'):
            members = by_group[bounds[g]:bounds[g + 1]]
            if len(members) >= 2 and usable[members[0]]:           # fewer than 2 rows make no transition (:464-466)
                episodes.append(members)
    all_lengths = [len(m) - 1 for m in episodes]
    first = surviving_episodes(all_lengths, max_size) if max_size is not None else 0
    kept = episodes[first:]
    lengths = all_lengths[first:]
    N = int(sum(lengths))
    src, src_next = np.empty(N, dtype=np.int32), np.empty(N, dtype=np.int32)
    last = np.zeros(N, dtype=np.uint8)
    t = 0
    for members, T in zip(kept, lengths):
        src[t:t + T], src_next[t:t + T] = members[:-1], members[1:]
        last[t + T - 1] = 1
        t += T
    return CsvTables(path=path, features=features, action=action, reward=reward, probabilities=probabilities,
                     src=src, src_next=src_next, last=last, episode_lengths=lengths, all_episode_lengths=all_lengths)


def write_csv_dataset(path, episodes, n_actions):
    """the schema above, one file row per state: episodes is a list of dicts of host arrays — obs [T, D], next_obs [T, D],
    action [T], reward [T], probabilities [T, A] or None.  An episode of T transitions gives T + 1 rows; the last carries
    the final next state with action 0, reward 0 and uniform probabilities (n_actions None: no probabilities column is
    written).  Every float is written with
    repr(float(x)): an fp32 value survives the round trip exactly."""
    D = episodes[0]["obs"].shape[1] if episodes else 0
    with open(path, "w", newline='') as f:
        w = csv.writer(f)
        w.writerow([EPISODE_ID, 'transition_number'] + ["%s_%d" % (STATE_PREFIX, k) for k in range(D)] +
                   [ACTION, REWARD] + ([PROBABILITIES] if n_actions else []))
        uniform = [1.0 / n_actions] * n_actions if n_actions else None
        for e, ep in enumerate(episodes):
            T = len(ep["action"])
            for i in range(T + 1):
                state = ep["obs"][i] if i < T else ep["next_obs"][T - 1]
                if i < T:
                    p = uniform if ep["probabilities"] is None else [float(x) for x in ep["probabilities"][i]]
                    a, r = int(ep["action"][i]), float(ep["reward"][i])
                else:
                    p, a, r = uniform, 0, 0.0
                w.writerow([e, i] + [repr(float(x)) for x in state] + [a, repr(r)] +
                           (["[" + ", ".join(repr(x) for x in p) + "]"] if n_actions else []))
