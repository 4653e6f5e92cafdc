"""rlx_adam_split_blocks / rlx_adam_step_blocks: which virtual blocks of the register-held Adam step may run early.

Pure host arithmetic, checked without a GPU against a ten-line model of the rule in include/rlx.h and, independently,
against the kernel's own element <-> (block, thread, iteration) mapping (csrc/adam_block_body.hpp)."""
import ctypes

import numpy as np
import pytest

from coach_amd import _rlx
from coach_amd.nn import graph as G
from coach_amd.nn.networks import build_torso

BLOCK, ITERS = 256, 4


def c2_params():
    """the Clipped-PPO Atari network's flat layout (ClippedPPONet's constructor, host part) -> (size, FC range)"""
    p = G.FlatParams()
    torso, feat = build_torso(p, "main", (84, 84, 4), "tanh", 2, "Medium", "Medium")
    G.Dense(p, "main/v_head/dense", feat, 1, None, 1)
    G.Dense(p, "main/ppo_head/policy_fc", feat, 6, None, 1)
    fc = [l for l in torso.layers if type(l) is G.Dense]
    assert len(fc) == 1 and (fc[0].K, fc[0].N) == (3136, 512)
    return p.size, fc[0].group_range()


C2_N, C2_FC = c2_params()


def step_blocks(n, workspace_floats=1 << 18):
    b = ctypes.c_int(-1)
    _rlx.lib().adam_step_blocks(n, workspace_floats, ctypes.byref(b))
    return b.value


def split(n, blocks, ranges):
    flat = (ctypes.c_longlong * max(1, 2 * len(ranges)))(*[x for r in ranges for x in r])
    early, late = (ctypes.c_int * blocks)(), (ctypes.c_int * blocks)()
    ne, nl = ctypes.c_int(), ctypes.c_int()
    _rlx.lib().adam_split_blocks(n, blocks, flat if ranges else None, len(ranges), early, ctypes.byref(ne), late, ctypes.byref(nl))
    return list(early[:ne.value]), list(late[:nl.value])


def model(n, blocks, ranges):
    n4, stride = n // 4, blocks * BLOCK
    early, late = [], []
    for vb in range(blocks):
        starts = [a for a in (vb * BLOCK + it * stride for it in range(ITERS)) if a < n4]
        runs = [(4 * a, 4 * min(a + BLOCK, n4)) for a in starts]
        ok = bool(runs) and not (vb == 0 and n % 4) and \
            all(any(r0 <= lo and hi <= r1 for r0, r1 in ranges) for lo, hi in runs)
        (early if ok else late).append(vb)
    if not late:                    # the finish needs a late workgroup
        late.append(early.pop())
    return early, late


def elements_of(vb, n, blocks):
    """every element the kernel's block vb touches (adam_block_body.hpp: float4 i = vb * 256 + t + it * blocks * 256)"""
    n4 = n // 4
    i = (vb * BLOCK + np.arange(BLOCK)[None, :] + np.arange(ITERS)[:, None] * blocks * BLOCK).ravel()
    el = (4 * i[i < n4][:, None] + np.arange(4)[None, :]).ravel()
    tail = 4 * n4 + vb * BLOCK + np.arange(BLOCK)
    return np.concatenate([el, tail[tail < n]])


def range_sets(n):
    third = n // 3
    sets = {
        "empty": [],
        "everything": [(0, n)],
        "mid_run": [(n // 7 + 3, n - n // 9 - 1)],                 # starts and ends inside a block's run
        "short": [(third, min(n, third + 500))],                     # shorter than one run of 1024 floats
        "two": [(0, n // 5), (n // 2 + 1, n - 2)],
    }
    if n == C2_N:
        sets["fc"] = [C2_FC]
    return sets


CASES = [(n, None) for n in (5, 1023, 4099, 1048579, C2_N)] + [(3000, 3), (4099, 2), (C2_N, 900)]   # (n, workspace cap)


@pytest.mark.parametrize("n,cap", CASES)
def test_split_matches_model_and_mapping(n, cap):
    blocks = step_blocks(n) if cap is None else step_blocks(n, cap)
    uncapped = min(1024, -(-(n // 4 + 1) // BLOCK))
    assert blocks == (uncapped if cap is None else min(uncapped, cap))
    for name, ranges in range_sets(n).items():
        early, late = split(n, blocks, ranges)
        assert (early, late) == model(n, blocks, ranges), name
        assert sorted(early + late) == list(range(blocks)), name          # every block, exactly once
        assert late, name
        inside = np.zeros(n, dtype=bool)
        for lo, hi in ranges:
            inside[lo:hi] = True
        for vb in early:
            assert inside[elements_of(vb, n, blocks)].all(), (name, vb)  # no early element outside the ranges
        if n % 4:
            assert 0 in late, name                                        # the owner of the tail elements
        if name == "empty":
            assert not early


def test_every_element_belongs_to_one_block():
    for n, blocks in ((5, 1), (4099, 5), (4099, 2), (3000, 3)):
        seen = np.concatenate([elements_of(vb, n, blocks) for vb in range(blocks)])
        assert sorted(seen.tolist()) == list(range(n))


def test_c2_fc_range_is_mostly_early():
    blocks = step_blocks(C2_N)
    assert blocks == 1024
    early, late = split(C2_N, blocks, [C2_FC])
    # the convolution parameters in front of the FC group and the heads behind it: about 160 of the 1024 blocks
    assert 100 < len(late) < 220 and len(early) + len(late) == 1024


def test_step_blocks_is_zero_where_the_register_form_does_not_fit():
    assert step_blocks(1048579, 1) == 0            # 262144 float4 in one block of 256 x 4
    assert step_blocks(5_000_000) == 0             # beyond 1024 x 256 x 4 float4
    with pytest.raises(_rlx.RlxError, match="do not fit"):
        split(1048579, 1, [])
