"""The GEMM dispatcher's launches, held to a recording: for one small seeded product per path, the kernels launched (their
names carry the template arguments) in launch order and a SHA-256 of every output's bytes must be those of
tests/golden/gemm_dispatch.json, recorded with this very code on an MI355X from the build BEFORE the dispatcher became
plan_gemm / launch_product / finish_product:

    python tests/test_gemm_dispatch.py gemm_dispatch.json          (from the root of the tree to record)
"""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDING = os.path.join(HERE, "golden", "gemm_dispatch.json")


def _t(rng, *shape, scale=1.0):
    import torch
    return torch.from_numpy((rng.randn(*shape) * scale).astype(np.float32)).to("cuda:0")


def _out(*shape):
    import torch
    return torch.full(shape, 7.0, dtype=torch.float32, device="cuda:0")


def _ws(floats=1 << 23):
    import torch
    return torch.empty(floats, dtype=torch.float32, device="cuda:0")


def _plain(M, N, K, batch=1, ws=True, **kw):
    """C[b] = A[b] B[b] through rlx_gemm (or rlx_gemm_defer + the jobs launch with defer=True)"""
    def run(rng):
        from coach_amd import _rlx
        A, B, C = _t(rng, batch, M, K), _t(rng, batch, K, N, scale=K ** -0.5), _out(batch, M, N)
        job = _rlx.SplitkJob() if kw.get("defer") else None
        _rlx.gemm(M, N, K, A, B, C, batch=batch, a_batch_stride=M * K, b_batch_stride=K * N, c_batch_stride=M * N,
                  workspace=_ws() if ws else None, **dict(kw, defer=job))
        if job is not None:
            assert job.splits > 1
            _rlx.splitk_reduce_jobs([job])
        return [C]
    return run


def _layer_grads(R, Kin, Nout, shared_ws=False, defer=False):
    """a dense layer's dW = X^T dY and dX = dY W^T as rlx_gemm_pair (or, alone=..., rlx_gemm on the dW descriptor)"""
    def descs(rng):
        from coach_amd import _rlx
        X, dY, W = _t(rng, R, Kin), _t(rng, R, Nout), _t(rng, Kin, Nout, scale=Nout ** -0.5)
        dW, dX, ws = _out(Kin, Nout), _out(R, Kin), _ws()
        dw = _rlx.gemm(Kin, Nout, R, X, dY, dW, a_strides=(1, Kin), workspace=ws, launch=False)
        dx = _rlx.gemm(R, Kin, Nout, dY, W, dX, b_strides=(1, Nout), workspace=ws if shared_ws else _ws(), launch=False)
        return dw, dx, [dW, dX], (X, dY, W, ws)

    def pair(rng):
        from coach_amd import _rlx
        dw, dx, outs, keep = descs(rng)
        job = _rlx.SplitkJob() if defer else None
        _rlx.gemm_pair(dw, dx, defer=job)
        if job is not None:
            assert job.splits > 1
            _rlx.splitk_reduce_jobs([job])
        return outs

    def alone(rng):
        from coach_amd import _rlx
        dw, dx, outs, keep = descs(rng)
        _rlx.gemm_pair_or_single(dw)
        return outs[:1]
    return pair, alone


def _conv_dws(both_through_tables):
    """two weight gradients as rlx_gemm_multi_defer: of convolutions (A^T gathered through im2col tables: one launch), or
    the second of a dense layer of the same shape (no tables: a launch each)"""
    def run(rng):
        import torch
        from coach_amd import _rlx
        B, H, W, C, KH, S, Co = 8, 84, 84, 4, 8, 4, 64
        OH = (H - KH) // S + 1
        M, K = B * OH * OH, KH * KH * C
        rowbase = torch.empty(M, dtype=torch.int32, device="cuda:0")
        koff = torch.empty(K, dtype=torch.int32, device="cuda:0")
        _rlx.lib().conv_tables(rowbase, koff, B, H, W, C, KH, KH, S, 0)
        x, ws = _t(rng, B, H, W, C), [_ws(), _ws()]
        dys, dws, jobs = [_t(rng, M, Co) for _ in range(2)], [_out(K, Co) for _ in range(2)], [_rlx.SplitkJob() for _ in range(2)]
        descs = [_rlx.gemm(K, Co, M, x, dys[i], dws[i], a_tabs=(koff, rowbase), a_vec_along_k=0, a_tab_vec_ok=1,
                           workspace=ws[i], launch=False) for i in range(2)]
        x2 = _t(rng, M, K)
        if not both_through_tables:
            descs[1] = _rlx.gemm(K, Co, M, x2, dys[1], dws[1], a_strides=(1, K), workspace=ws[1], launch=False)
        _rlx.gemm_multi(descs, jobs)
        assert all(j.splits > 1 for j in jobs)
        _rlx.splitk_reduce_jobs(jobs)
        return dws
    return run


def _row_heads(M, N, K, batch, head_n):
    """tests/test_gemm.py's row_heads product: the last dense layer with the narrow layers that read its rows"""
    def run(rng):
        from coach_amd import _rlx
        A, B, bias = _t(rng, batch, M, K), _t(rng, batch, K, N, scale=K ** -0.5), _t(rng, batch, N)
        hw, hb = [_t(rng, N, n, scale=N ** -0.5) for n in head_n], [_t(rng, n) for n in head_n]
        C, ys = _out(batch, M, N), [_out(M, n) for n in head_n]
        arr = (_rlx.SmallDenseProblem * len(head_n))()
        for i, n in enumerate(head_n):
            q = arr[i]
            q.x, q.w, q.bias, q.y = C.data_ptr() + i * M * N * 4, hw[i].data_ptr(), hb[i].data_ptr(), ys[i].data_ptr()
            q.y_tower_stride, q.towers, q.M, q.K, q.N, q.activation = M * n, 1, M, N, n, 0
        _rlx.gemm(M, N, K, A, B, C, bias=bias, activation="relu", batch=batch, a_batch_stride=M * K, b_batch_stride=K * N,
                  c_batch_stride=M * N, bias_batch_stride=N, workspace=_ws(), row_heads=arr)
        return [C] + ys
    return run


def _folded(M, K, N, T):
    """T towers reading the same A as one product over T * N columns (n_fold), forward with bias and activation"""
    def run(rng):
        from coach_amd import _rlx
        A, W, b, y = _t(rng, M, K), _t(rng, T, K, N, scale=K ** -0.5), _t(rng, T, N), _out(T, M, N)
        _rlx.gemm(M, T * N, K, A, W, y, b_strides=(N, 1), ldc=N, bias=b, activation="tanh", batch=1, b_batch_stride=K * N,
                  c_batch_stride=M * N, bias_batch_stride=N, workspace=_ws(), n_fold=N)
        return [y]
    return run


def cases():
    thin_pair, thin16_alone = _layer_grads(100, 400, 300)               # dW 400 x 300 x 100: 130 tiles of 32 x 32
    ring_pair, _ = _layer_grads(3136, 512, 256, defer=True)
    clash_pair, _ = _layer_grads(2048, 512, 256, shared_ws=True)        # both halves split K into one workspace: two launches
    return {
        "thin32": _plain(512, 768, 64),
        "thin16_alone": thin16_alone,
        "thin_pair": thin_pair,
        "generic_scalar_reduce": _plain(512, 510, 2048),
        "fast_ring": _plain(3136, 512, 256, ws=False),
        "fast_register_staged_narrow_reduce_3": _plain(25600, 32, 256),
        "reduce_25": _plain(64, 512, 3136, batch=2),
        "deferred_reduce_25": _plain(64, 512, 3136, batch=2, defer=True),
        "kw2": _plain(3136, 64, 576, batch=2),
        "kw4": _plain(3136, 64, 2048),
        "kw4_by_hint": _plain(32, 3136, 512, kw_min_tiles=96),
        "big_128x128": _plain(2048, 2048, 64),
        "ring_pair_deferred": ring_pair,
        "pair_falls_back_on_a_shared_workspace": clash_pair,
        "multi_one_launch": _conv_dws(True),
        "multi_falls_back_without_tables": _conv_dws(False),
        "row_heads_in_the_reduction": _row_heads(64, 512, 3136, 2, (1, 6)),
        "row_heads_behind_the_reduction": _row_heads(64, 512, 1056, 2, (1, 6)),        # 11 chunks: the plain reduction
        "row_heads_behind_a_thin_product": _row_heads(64, 512, 320, 2, (1, 6)),
        "n_fold": _folded(256, 64, 32, 2),
        "n_fold_falls_back": _folded(100, 23, 20, 2),
    }


def run_all():
    """{case: {"kernels": names in launch order, "sha256": one digest per output}}"""
    import torch
    from coach_amd import _rlx
    lib = _rlx.lib()
    lib.gemm_tuning(192, 192, -1), lib.gemm_split_cap(64), lib.gemm_pipeline(1), lib.gemm_big_tiles(1)     # the defaults
    got = {}
    for name, run in sorted(cases().items()):
        with _rlx.KernelTimer(64) as timer:
            outs = run(np.random.RandomState(0))
        torch.cuda.synchronize()
        got[name] = {"kernels": [n for n, _ in timer.records],
                     "sha256": [hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest() for o in outs]}
    return got


@pytest.mark.gpu
def test_every_path_launches_and_computes_what_the_recording_holds():
    with open(RECORDING) as f:
        recorded = json.load(f)
    got = run_all()
    assert sorted(got) == sorted(recorded)
    wrong = {k: (got[k], recorded[k]) for k in recorded if got[k] != recorded[k]}
    assert not wrong, "(this build, the recording): %r" % wrong
    # the recording itself: every path of the list above is in it
    names = {k: " ".join(v["kernels"]) for k, v in recorded.items()}
    for case, parts in {
            "thin32": ["gemm_thin_kernel<"], "thin16_alone": ["gemm_thin16_kernel<"], "thin_pair": ["gemm_thin_pair_kernel"],
            "generic_scalar_reduce": ["gemm_kernel<", "splitk_reduce_kernel"], "fast_ring": ["gemm_dma_kernel<"],
            "fast_register_staged_narrow_reduce_3": ["gemm_fast_kernel<", "splitk_reduce4_kernel<4>"],
            "reduce_25": ["splitk_reduce4_kernel<16>"], "deferred_reduce_25": ["splitk_reduce_jobs_kernel"],
            "kw2": ["gemm_dma_kernel<"], "kw4": ["gemm_dma_kernel<"], "kw4_by_hint": ["gemm_dma_kernel<"],
            "big_128x128": ["gemm_dma_big_kernel<"], "ring_pair_deferred": ["gemm_dma_pair_kernel<false, 1>", "splitk_reduce_jobs_kernel"],
            "pair_falls_back_on_a_shared_workspace": ["gemm_dma_kernel<", "splitk_reduce4_kernel<"],
            "multi_one_launch": ["gemm_multi_dw_kernel"], "multi_falls_back_without_tables": ["gemm_dma_kernel<"],
            "row_heads_in_the_reduction": ["splitk_reduce_rows_kernel<"], "row_heads_behind_the_reduction": ["splitk_reduce4_kernel<4>", "dense_small_fwd"],
            "row_heads_behind_a_thin_product": ["gemm_thin16_kernel<", "dense_small_fwd"],
            "n_fold": ["gemm_"], "n_fold_falls_back": ["gemm_thin"]}.items():
        for part in parts:
            assert part in names[case], (case, names[case])
    assert len(recorded["thin16_alone"]["kernels"]) == 1 and len(recorded["kw2"]["kernels"]) == 1
    assert len(recorded["pair_falls_back_on_a_shared_workspace"]["kernels"]) == 4
    assert "pair" not in names["pair_falls_back_on_a_shared_workspace"] and "multi" not in names["multi_falls_back_without_tables"]
    # thin 16 alone against the same product inside the pair: same sums, so the same bytes
    assert recorded["thin16_alone"]["sha256"][0] == recorded["thin_pair"]["sha256"][0]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    with open(sys.argv[1], "w") as f:
        f.write(json.dumps(run_all(), indent=0, sort_keys=True) + "\n")
    print("recorded", sys.argv[1])
