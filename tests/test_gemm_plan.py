"""The GEMM dispatcher's plan, held to a recording: rlx_gemm_describe and rlx_ppo_fc_rows_supported must answer for every
descriptor of tests/golden/make_gemm_plans.py's table what the build BEFORE the dispatcher was restructured answered
(tests/golden/gemm_plans.json).  Host code only: runs without a GPU."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_gemm_plans", os.path.join(GOLDEN, "make_gemm_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def gen():
    return _generator()


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "gemm_plans.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def answered(gen):
    return gen.answers()


def test_the_table_and_the_recording_hold_the_same_cases(gen, recorded):
    assert sorted(c["name"] for c in gen.CASES) == sorted(recorded)


def test_every_plan_equals_the_recording(answered, recorded):
    wrong = {k: (answered[k], recorded[k]) for k in recorded if answered.get(k) != recorded[k]}
    assert not wrong, "(this build, the recording): %r" % wrong


def test_the_generator_reproduces_the_file_byte_for_byte(gen, answered):
    with open(os.path.join(GOLDEN, "gemm_plans.json")) as f:
        assert gen.render(answered) == f.read()


def test_the_issue_reference_answers(recorded):
    """the answers read from the build before the restructuring, as the issue lists them"""
    want = {"fc_forward_split25": [1, 64, 64, 1, 25, 128, 1, 0], "kw2": [1, 32, 64, 2, 1, 576, 1, 0],
            "kw4": [1, 32, 32, 4, 1, 2048, 1, 0], "narrow_n32": [1, 128, 32, 1, 3, 96, 0, 0],
            "n_not_multiple_of_4": [0, 64, 64, 1, 8, 256, 0, 0], "thin_400x300x100": [0, 0, 0, 0, 0, 0, 0, 1],
            # a launch of its own takes 128 x 128 wave tiles here; describe answers for the (bit-identical) 64 x 64 tiling
            "big_candidate_4096": [1, 64, 64, 1, 1, 512, 1, 0], "big_candidate_2048": [1, 64, 64, 1, 1, 64, 1, 0]}
    assert {k: recorded[k]["describe"] for k in want} == want


def test_the_table_reaches_both_sides_of_the_selection(recorded):
    """what the recording must contain for the table to mean anything: every tile, wave-group count, both pipelines, the
    thin and the generic path, split and unsplit, a capped split, a refused and a fallen-back fold"""
    d = [v["describe"] for v in recorded.values()]
    plans = [x for x in d if isinstance(x, list)]
    assert {(x[1], x[2], x[3]) for x in plans if x[0]} == {(64, 64, 1), (128, 32, 1), (32, 64, 2), (32, 32, 4)}
    assert {x[6] for x in plans if x[0]} == {0, 1} and {x[0] for x in plans if not x[7]} == {0, 1}
    assert any(x[7] for x in plans) and any(x == [0] * 8 for x in plans)
    assert {1, 10, 16, 25, 64} <= {x[4] for x in plans}
    assert any(isinstance(x, str) and "n_fold" in x for x in d)
    assert {v["ppo_fc_rows_supported"] for v in recorded.values()} == {0, 1}


def test_the_knobs_are_back_at_their_defaults(gen, answered):
    import ctypes
    from coach_amd import _rlx
    lib = _rlx.lib()
    below, least, xcd = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    lib.gemm_tuning_get(ctypes.byref(below), ctypes.byref(least), ctypes.byref(xcd))
    assert (below.value, least.value, xcd.value) == (192, 192, -1)
    # split cap, pipeline and big tiles have no getters: a descriptor each of them decides must plan as by default
    by_name = {c["name"]: c for c in gen.CASES}
    for name, want in (("split_cap_64", 64), ("fp32_pipeline1", None), ("u8_tabs_pipeline1", None)):
        q = (ctypes.c_int * 8)()
        lib.gemm_describe(ctypes.byref(gen.descriptor(_rlx, by_name[name])), q)
        assert list(q) == answered[name]["describe"]
        assert want is None or q[4] == want
