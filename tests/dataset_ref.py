"""Numpy restatement of rlx_dataset_ingest (coach_amd/csrc/dataset.hip), bit for bit: the flat tables of
coach_amd/memories/episodic/csv_dataset.py -> the replay rows the launch writes.  Pinned to the reference's own
EpisodicExperienceReplay.load_csv by tests/test_dataset_ref.py (tests/golden/dataset.npz)."""
import numpy as np

STATUS_ACTION, STATUS_NOT_FINITE, STATUS_INDEX = 1, 2, 4


def reward_filter(rewards32, rescale=1.0, clip=None):
    """rlx_reward_filter on fp32 rewards: fp64 product, then the clipping filter's truthiness (a bound of 0 is not
    applied; fmin / fmax drop a NaN), rounded to fp32 once"""
    r = np.asarray(rewards32, dtype=np.float32).astype(np.float64) * np.float64(rescale)
    if clip is not None:
        lo, hi = clip
        if hi != 0.0:
            r = np.fmin(r, np.float64(hi))
        if lo != 0.0:
            r = np.fmax(r, np.float64(lo))
    with np.errstate(over="ignore"):
        return r.astype(np.float32)


def ingest(features, action, reward, probabilities, src, src_next, last, is_episodic, n_actions, rescale=1.0,
           clip=None):
    """-> dict(obs, next_obs fp32 [N, D]; action int32 [N]; reward fp32 [N]; game_over uint8 [N]; probabilities fp32
    [N, A] or None; status).  Leading dimensions are not modelled: pass the used columns."""
    features = np.asarray(features, dtype=np.float64)
    R = features.shape[0]
    src, src_next = np.asarray(src, dtype=np.int64), np.asarray(src_next, dtype=np.int64)
    ok, ok_next = (src >= 0) & (src < R), (src_next >= 0) & (src_next < R)
    s, sn = np.where(ok, src, 0), np.where(ok_next, src_next, 0)
    with np.errstate(over="ignore"):
        f32 = features.astype(np.float32)                         # round to nearest even, once
        r32 = np.asarray(reward, dtype=np.float64).astype(np.float32)
    obs = np.where(ok[:, None], f32[s], np.float32(0))
    next_obs = np.where(ok_next[:, None], f32[sn], np.float32(0))
    a = np.where(ok, np.asarray(action, dtype=np.int32)[s], 0).astype(np.int32)
    bad_action = (a < 0) | (a >= n_actions)
    a[bad_action] = 0
    r = np.where(ok, r32[s], np.float32(0)).astype(np.float32)
    status = 0
    if bad_action.any():
        status |= STATUS_ACTION
    if not (np.isfinite(obs).all() and np.isfinite(next_obs).all() and np.isfinite(r).all()):
        status |= STATUS_NOT_FINITE
    if not (ok.all() and ok_next.all()):
        status |= STATUS_INDEX
    probs = None
    if probabilities is not None:
        probs = np.where(ok[:, None], np.asarray(probabilities, dtype=np.float32)[s], np.float32(0))
    game_over = ((np.asarray(last) != 0) & bool(is_episodic)).astype(np.uint8)
    return dict(obs=obs, next_obs=next_obs, action=a, reward=reward_filter(r, rescale, clip), game_over=game_over,
                probabilities=probs, status=status)


def episode_returns(rewards32, lengths, discount=0.99):
    """n_step_discounted_rewards of episodes built by load_csv — Episode() with its defaults, discount 0.99 and n_step -1
    (core_types.py:771-801), in the reference's summation order — from the stored fp32 rewards -> fp64 [N]"""
    out, first = [], 0
    for T in lengths:
        rewards = np.asarray(rewards32[first:first + T], dtype=np.float32).astype('float')
        discounted_rewards = rewards.copy()
        current_discount = discount
        for i in range(1, T):
            discounted_rewards += current_discount * np.pad(rewards[i:], (0, i), 'constant', constant_values=0)
            current_discount *= discount
        out.append(discounted_rewards)
        first += T
    return np.concatenate(out)
