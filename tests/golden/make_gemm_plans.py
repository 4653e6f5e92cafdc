#!/usr/bin/env python
"""Generate tests/golden/gemm_plans.json: what rlx_gemm_describe and rlx_ppo_fc_rows_supported answer for a table of
descriptors and knob settings.  Both are host-only (they plan, they launch nothing and never read the operands), so the
descriptors carry made-up, aligned pointers and the script runs without a GPU.  Run from the root of the tree whose
library is to be recorded (it drives that tree's coach_amd/librlx.so):

    python tests/golden/make_gemm_plans.py [output.json]

The committed file was recorded from a build of the commit BEFORE the dispatcher became plan_gemm / launch_product /
finish_product; tests/test_gemm_plan.py holds every later build to it.  CASES puts a descriptor on each side of every
branch of the selection (csrc/gemm.hip plan_desc); a new branch needs new cases and a recording from the build before it.
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEFAULT_OUT = os.path.join(ROOT, "tests", "golden", "gemm_plans.json")

A, B, C, WS, TAB = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000   # made up, 16-byte aligned
KNOBS = {"tuning": (192, 192), "split_cap": 64, "pipeline": 1, "big_tiles": 1}   # the library's defaults
N_ACTIONS = 6


def case(name, M, N, K, batch=1, ws="plenty", knobs=None, **opts):
    return {"name": name, "shape": (M, N, K, batch), "ws": ws, "knobs": dict(KNOBS, **(knobs or {})), "opts": opts}


def _cases():
    c = [
        # --- the issue's reference answers
        case("fc_forward_split25", 64, 512, 3136, 2),
        case("kw2", 3136, 64, 576, 2),
        case("kw4", 3136, 64, 2048, 1),
        case("narrow_n32", 25600, 32, 256, 1),
        case("n_not_multiple_of_4", 512, 510, 2048, 1),
        case("thin_400x300x100", 400, 300, 100, 1),
        case("big_candidate_4096", 4096, 4096, 512, 1),
        case("big_candidate_2048", 2048, 2048, 64, 1),
        case("big_candidate_2048_tiles0", 2048, 2048, 64, 1, knobs={"big_tiles": 0}),
        case("big64_candidate_tiles2", 65536, 64, 64, 1, knobs={"big_tiles": 2}),
        # --- thin limits: 96 tiles of 64 x 64, N * K <= 2^18, K <= 1024
        case("thin_96_tiles", 384, 64, 128, 16),
        case("thin_102_tiles", 384, 64, 128, 17),
        case("thin_nk_at_limit", 64, 512, 512, 1),
        case("thin_nk_over_limit", 64, 512, 516, 1),
        case("thin_k_1024", 64, 64, 1024, 1),
        case("thin_k_1028", 64, 64, 1028, 1),
        case("thin_sized_but_u8", 64, 64, 256, 1, a_u8=True),
        # --- in-workgroup K split: below / min tiles at the defaults, another setting, the per-descriptor hint
        case("kw_191_tiles", 12224, 64, 256, 1),
        case("kw_192_tiles", 12288, 64, 256, 1),
        case("kw_off", 3136, 64, 576, 2, knobs={"tuning": (0, 192)}),
        case("kw2_min_200", 3136, 64, 576, 2, knobs={"tuning": (192, 200)}),
        case("kw4_min_200", 3136, 64, 2048, 1, knobs={"tuning": (192, 200)}),
        case("kw_below_256_min_64", 12288, 64, 256, 1, knobs={"tuning": (256, 64)}),
        case("kw_hint_96", 32, 3136, 512, 1, kw_min_tiles=96),
        case("kw_no_hint", 32, 3136, 512, 1),
        case("kw_hint_99", 32, 3136, 512, 1, kw_min_tiles=99),
        case("kw_not_for_transposed_tables", 3136, 64, 576, 2, tabs=True, b_t=True),
        # --- split heuristic: at most 256 tiles, K / 64, the cap at 64 and 16, a workspace too small, none
        case("split_256_tiles", 16384, 64, 2048, 1),
        case("split_257_tiles", 16448, 64, 2048, 1),
        case("split_bound_by_k", 128, 2048, 256, 1),
        case("split_k_127", 128, 2048, 127, 1),
        case("split_cap_64", 64, 512, 16384, 1),
        case("split_cap_16", 64, 512, 16384, 1, knobs={"split_cap": 16}),
        case("split_cap_64_one_tile", 64, 64, 16384, 1),
        case("split_ws_for_10", 64, 512, 16384, 1, ws=(64 * 512 + 512) * 10),
        case("split_ws_for_1", 64, 512, 16384, 1, ws=100),
        case("split_no_ws", 64, 512, 16384, 1, ws=None),
        case("split_ws_misaligned", 64, 512, 16384, 1, ws_off=4),
        # --- tile and layout: narrow N, A through tables around the LDS table bounds (no workspace: one chunk)
        case("narrow_n36", 25600, 36, 256, 1),
        case("narrow_n32_no_ws", 25600, 32, 256, 1, ws=None),
        case("tabs_chunk_2048", 3136, 64, 2048, 2, ws=None, tabs=True),
        case("tabs_chunk_2080", 3136, 64, 2080, 2, ws=None, tabs=True),
        case("tabs_chunk_2080_narrow", 25600, 32, 2080, 1, ws=None, tabs=True),
        case("tabs_split", 3136, 64, 4096, 1, tabs=True),
        case("tabs_vec_along_rows", 576, 64, 3136, 2, tabs=True, a_vec_along_k=0),
        case("tabs_no_vectors", 3136, 64, 576, 2, tabs=True, a_tab_vec_ok=0),
        case("one_table_only", 3136, 64, 576, 2, tabs="row"),
        # --- uint8 A under the three pipelines
    ]
    for mode in (0, 1, 2):
        c += [
            case("u8_tabs_pipeline%d" % mode, 3136, 64, 256, 8, tabs=True, a_u8=True, knobs={"pipeline": mode}),
            case("u8_tabs_narrow_pipeline%d" % mode, 25600, 32, 256, 1, tabs=True, a_u8=True, knobs={"pipeline": mode}),
            case("u8_plain_pipeline%d" % mode, 3136, 512, 256, 1, a_u8=True, knobs={"pipeline": mode}),
            case("fp32_pipeline%d" % mode, 3136, 512, 256, 1, knobs={"pipeline": mode}),
            case("fp32_tabs_pipeline%d" % mode, 3136, 64, 2048, 2, ws=None, tabs=True, knobs={"pipeline": mode}),
        ]
    c += [
        # --- towers folded into N: qualifying, falling back (each reason), refused
        case("fold_ok", 3136, 128, 576, 1, n_fold=64),
        case("fold_ok_split", 64, 1024, 3136, 1, n_fold=512),
        case("fold_not_multiple_of_4", 3136, 124, 576, 1, n_fold=62),
        case("fold_transposed_b", 3136, 128, 576, 1, n_fold=64, b_t=True),
        case("fold_accumulate", 3136, 128, 576, 1, n_fold=64, accumulate=True),
        case("fold_not_fast", 3135, 128, 576, 1, n_fold=64, a_t=True),
        case("fold_n_not_divisible", 3136, 128, 576, 1, n_fold=48),
        case("fold_batch_2", 3136, 128, 576, 2, n_fold=64),
        # --- operands: transposed B / A, misaligned pointers, M / N / K not multiples of 4
        case("b_transposed", 3136, 512, 576, 1, b_t=True),
        case("a_transposed", 3136, 512, 576, 1, a_t=True),
        case("a_transposed_m_odd", 3135, 512, 576, 1, a_t=True),
        case("a_misaligned", 3136, 512, 576, 1, a_off=4),
        case("b_misaligned", 3136, 512, 576, 1, b_off=8),
        case("c_misaligned", 3136, 512, 576, 1, ws=None, c_off=4),
        case("bias_misaligned", 3136, 512, 576, 1, ws=None, bias_off=4),
        case("m_odd", 3135, 512, 576, 1),
        case("k_odd", 3136, 512, 575, 1),
        case("k_3", 3136, 512, 3, 1),
        case("thin_transposed", 100, 300, 400, 1, a_t=True),
        case("bad_shape", 0, 512, 576, 1),
        case("bad_activation", 64, 512, 576, 1, activation=3),
        case("u8_without_a_div", 3136, 512, 256, 1, a_u8=True, a_div=0.0),
        case("batch_inner_mismatch", 64, 512, 3136, 3, batch_inner=2),
        # --- rlx_ppo_fc_rows_supported: more than 16 chunks or not, and its own limits
        case("ppo_rows_25_chunks", 32, 512, 3136, 2),
        case("ppo_rows_16_chunks", 32, 512, 3136, 2, knobs={"split_cap": 16}),
        case("ppo_rows_thin", 32, 64, 256, 2),
        case("ppo_rows_m_257", 257, 512, 3136, 2),
        case("ppo_rows_n_1028", 32, 1028, 3136, 2),
        case("ppo_rows_batch_1", 32, 512, 3136, 1),
        case("ppo_rows_colsum", 32, 512, 3136, 2, colsum=True),
    ]
    return c


CASES = _cases()


def descriptor(_rlx, cs):
    M, N, K, batch = cs["shape"]
    o = cs["opts"]
    kw = {}
    if o.get("tabs"):
        kw["a_tabs"] = (TAB, TAB + (1 << 20) if o["tabs"] is True else None)
        kw["a_vec_along_k"], kw["a_tab_vec_ok"] = o.get("a_vec_along_k", 1), o.get("a_tab_vec_ok", 1)
    elif o.get("a_t"):
        kw["a_strides"] = (1, M)
    if o.get("b_t"):
        kw["b_strides"] = (1, K)
    fold = o.get("n_fold", 0)
    d = _rlx.gemm(M, N, K, A + o.get("a_off", 0), B + o.get("b_off", 0), C + o.get("c_off", 0), batch=batch,
                  a_batch_stride=M * K, b_batch_stride=K * (fold or N), c_batch_stride=M * (fold or N),
                  bias=(WS - (1 << 20) + o["bias_off"]) if "bias_off" in o else None, bias_batch_stride=fold or N,
                  a_u8=o.get("a_u8", False), a_div=o.get("a_div", 255.0 if o.get("a_u8") else 1.0),
                  accumulate=o.get("accumulate", False), batch_inner=o.get("batch_inner", 0), n_fold=fold,
                  kw_min_tiles=o.get("kw_min_tiles", 0), colsum_out=(WS - (1 << 21)) if o.get("colsum") else None,
                  colsum_batch_stride=N, launch=False, **kw)
    d.activation = o.get("activation", 0)
    if cs["ws"] is not None:
        d.workspace = WS + o.get("ws_off", 0)
        d.workspace_floats = (1 << 28) if cs["ws"] == "plenty" else int(cs["ws"])
    return d


def set_knobs(lib, k):
    lib.gemm_tuning(k["tuning"][0], k["tuning"][1], -1)
    lib.gemm_split_cap(k["split_cap"])
    lib.gemm_pipeline(k["pipeline"])
    lib.gemm_big_tiles(k["big_tiles"])


def answers():
    """{case name: {"describe": the eight outputs, or the library's error text; "ppo_fc_rows_supported": 0 / 1}} under
    each case's knobs; the knobs are back at the library's defaults afterwards."""
    sys.path.insert(0, ROOT)
    from coach_amd import _rlx
    lib = _rlx.lib()
    out = {}
    try:
        for cs in CASES:
            assert cs["name"] not in out, cs["name"]
            set_knobs(lib, cs["knobs"])
            d = descriptor(_rlx, cs)
            q = (ctypes.c_int * 8)(*([-1] * 8))
            try:
                lib.gemm_describe(ctypes.byref(d), q)
                described = list(q)
            except _rlx.RlxError as e:
                described = str(e)
            out[cs["name"]] = {"describe": described,
                               "ppo_fc_rows_supported": int(lib.ppo_fc_rows_supported(ctypes.byref(d), N_ACTIONS))}
    finally:
        set_knobs(lib, KNOBS)
    return out


def render(a):
    return json.dumps(a, indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else DEFAULT_OUT
    with open(path, "w") as f:
        f.write(render(answers()))
    print("%s: %d cases" % (path, len(CASES)))
