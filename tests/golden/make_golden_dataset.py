#!/usr/bin/env python
"""Generate tests/golden/dataset.npz by running the REFERENCE's own EpisodicExperienceReplay.load_csv (pandas) under the
stub-import harness (_refstub.py) on the committed CSV texts tests/golden/dataset_*.csv, in the manner of
make_golden_bcq.py.  Run from the repo root where the reference tree and pandas are present:

    python tests/golden/make_golden_dataset.py

Per case of CASES (file, is_episodic, max_size, reward filter) the reference memory's contents after load_csv are
recorded: <case>_states / _next_states (fp64 [N, D]), _actions, _rewards (fp64, after the input filter), _game_overs,
_probabilities (fp64 [N, A]), _episode_lengths, _returns (every transition's n_step_discounted_rewards), and what _split_training_and_evaluation_datasets makes of them at
train_to_eval_ratio 0.6 (_episode_id, _transition_id); "cases" lists the cases' parameters as JSON text.

Two things are asserted while generating.  For every numeric cell of every file, pandas' value and Python's float(text)
agree after the cast to fp32 (how many differ as doubles is printed): the product parses with float().  And for every
recorded reward, rounding the file's reward to fp32 BEFORE the filter's fp64 arithmetic — what the device does, like the
acting path, which stores an environment's fp32 reward — gives the fp32 value the reference's all-double arithmetic rounds
to.  That holds for every reward that is an fp32 value (an environment's logged reward usually is), and the filter cases
use the file whose rewards are.  For a reward that is not, the product is rounded twice where the reference rounds once,
and the fp32 results can differ in their last place: how many of dataset_basic.csv's rewards would under the rescale
filter is printed.
"""
import csv
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE), HERE]
import _refstub  # noqa: E402

_refstub.install()

import dataset_ref  # noqa: E402

# name: (file, is_episodic, (granularity, size), reward filter: None | ("rescale", factor) | ("clip", low, high))
CASES = {
    "episodic": ("dataset_basic.csv", True, ("Transitions", 1000000), None),
    "not_episodic": ("dataset_basic.csv", False, ("Transitions", 1000000), None),
    "transitions_9": ("dataset_long.csv", True, ("Transitions", 9), None),
    "episodes_2": ("dataset_long.csv", True, ("Episodes", 2), None),
    "rescale": ("dataset_long.csv", True, ("Transitions", 1000000), ("rescale", 1 / 200.)),
    "clip": ("dataset_long.csv", True, ("Transitions", 1000000), ("clip", -0.5, 2.0)),
}
RATIO = 0.6


def check_parsers(path):
    import pandas as pd
    df = pd.read_csv(path)
    with open(path, newline='') as f:
        rows = list(csv.reader(f))
    header, rows = rows[0], rows[1:]
    cells = differ = 0
    for j, name in enumerate(header):
        if not (name.startswith("state_feature") or name in ("action", "reward")):
            continue
        for i, r in enumerate(rows):
            mine, theirs = float(r[j]), float(df[name].iloc[i])
            cells += 1
            differ += mine != theirs
            assert np.float32(mine) == np.float32(theirs) and \
                np.float32(mine).tobytes() == np.float32(theirs).tobytes(), (path, name, i, r[j])
    print("%s: %d numeric cells, %d differ between pandas and float() as doubles, none as fp32"
          % (os.path.basename(path), cells, differ))


def run_case(name, file, is_episodic, max_size, flt):
    from rl_coach.core_types import CsvDataset
    from rl_coach.filters.filter import InputFilter
    from rl_coach.filters.reward.reward_clipping_filter import RewardClippingFilter
    from rl_coach.filters.reward.reward_rescale_filter import RewardRescaleFilter
    from rl_coach.memories.episodic.episodic_experience_replay import EpisodicExperienceReplay
    from rl_coach.memories.memory import MemoryGranularity
    mem = EpisodicExperienceReplay((MemoryGranularity[max_size[0]], max_size[1]), train_to_eval_ratio=RATIO)
    input_filter = InputFilter(is_a_reference_filter=False)
    if flt is not None and flt[0] == "rescale":
        input_filter.add_reward_filter('rescale', RewardRescaleFilter(flt[1]))
    elif flt is not None:
        input_filter.add_reward_filter('clip', RewardClippingFilter(flt[1], flt[2]))
    mem.load_csv(CsvDataset(os.path.join(HERE, file), is_episodic), input_filter)
    tr = mem.transitions
    assert len(tr) == mem.num_transitions_in_complete_episodes() == mem.num_transitions()
    out = {
        "states": np.array([t.state['observation'] for t in tr], dtype=np.float64),
        "next_states": np.array([t.next_state['observation'] for t in tr], dtype=np.float64),
        "actions": np.array([t.action for t in tr], dtype=np.int64),
        "rewards": np.array([t.reward for t in tr], dtype=np.float64),
        "game_overs": np.array([bool(t.game_over) for t in tr]),
        "probabilities": np.array([t.info['all_action_probabilities'] for t in tr], dtype=np.float64),
        "episode_lengths": np.array([e.length() for e in mem.get_all_complete_episodes()], dtype=np.int64),
        # store_episode -> close_last_episode -> Episode.update_transitions_rewards_and_bootstrap_data: load_csv's
        # Episode() has the class defaults, discount 0.99 and n_step -1
        "returns": np.array([t.n_step_discounted_rewards for t in tr], dtype=np.float64),
    }
    assert all(type(t.action) is int for t in tr)
    mem._split_training_and_evaluation_datasets()
    out["episode_id"] = np.int64(mem.get_last_training_set_episode_id())
    out["transition_id"] = np.int64(mem.last_training_set_transition_id)
    try:                                                           # (:447) a frozen memory does not load
        mem.freeze()
        mem.load_csv(CsvDataset(os.path.join(HERE, file), is_episodic), input_filter)
        raise SystemExit("a frozen memory loaded a file")
    except AssertionError as e:
        out["frozen_error"] = np.array(str(e))
    print("case %s: %d transitions in episodes of %s, training set = episodes 0..%d = %d transitions"
          % (name, len(tr), out["episode_lengths"].tolist(), out["episode_id"], out["transition_id"]))
    return out


def check_fp32_first(name, file, flt, recorded_rewards, n_transitions):
    """the device rounds the file's reward to fp32 before the filter: the same fp32 value as the reference's doubles?"""
    from coach_amd.memories.episodic.csv_dataset import read_csv_dataset
    t = read_csv_dataset(os.path.join(HERE, file), 1, False)
    assert t.n_transitions >= n_transitions
    src = t.src[t.n_transitions - n_transitions:]
    rescale, clip = 1.0, None
    if flt is not None and flt[0] == "rescale":
        rescale = flt[1]
    elif flt is not None:
        clip = (flt[1], flt[2])
    mine = dataset_ref.reward_filter(t.reward[src].astype(np.float32), rescale, clip)
    theirs = recorded_rewards.astype(np.float32)
    assert mine.tobytes() == theirs.tobytes(), (name, mine, theirs)


def count_double_rounding(file, rescale):
    from coach_amd.memories.episodic.csv_dataset import read_csv_dataset
    r = read_csv_dataset(os.path.join(HERE, file), 1, False).reward
    first = dataset_ref.reward_filter(r.astype(np.float32), rescale)
    once = (r * rescale).astype(np.float32)
    print("%s under rescale %r: %d of %d rewards differ in the last place of fp32 when rounded to fp32 first (%d are not "
          "fp32 values)" % (file, rescale, int((first != once).sum()), len(r), int((r.astype(np.float32) != r).sum())))


def main():
    for file in sorted({c[0] for c in CASES.values()}):
        check_parsers(os.path.join(HERE, file))
    out = {"cases": np.array(json.dumps(CASES, sort_keys=True)), "ratio": np.float64(RATIO)}
    for name, (file, is_episodic, max_size, flt) in CASES.items():
        rec = run_case(name, file, is_episodic, max_size, flt)
        check_fp32_first(name, file, flt, rec["rewards"], len(rec["rewards"]))
        for k, v in rec.items():
            out[name + "_" + k] = v
    count_double_rounding("dataset_basic.csv", 1 / 200.)
    path = os.path.join(HERE, "dataset.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %.1f KiB)" % (path, len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
