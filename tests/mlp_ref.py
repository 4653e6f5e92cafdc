"""float64 reference of the whole one-launch MLP DQN update (csrc/mlp_fused.hip: rlx_mlp_dqn_update) and of the acting
step's forward pass, in plain numpy, taking the fp32 weights as they are.

  obs -> Dense(H1, relu) -> Dense(H2, relu) -> Dense(A)                       (CartPole_DQN's network)
  TD targets of DQNAgent.learn_from_batch (dqn_agent.py:92-111), DQN and Double DQN, selection by np.argmax (first
  maximum, first NaN); MSE / Huber head loss with importance weights, mean over B (head.py:172-181); the gradients of
  all six tensors, the relu backward as dy * (y > 0) -- a MULTIPLICATION, as in oracle/nn.py and rlx::act_deriv_out:
  a NaN or inf gradient at an inactive unit is NaN, not 0.

Next to every pre-activation and Q value stands an a-priori bound on what an fp32 evaluation, in any summation order,
can differ from it: (K + 2) * 2^-24 * (sum_k |x_k w_k| + |b|) for the layer's own arithmetic plus the bounds of its
inputs carried through |W|.  The seeded cases of tests/test_mlp_fused_edges.py are built here (CASES, make_case) so that
tests/test_mlp_ref.py can assert on the CPU that none of their discontinuities -- the sign of a pre-activation, the
arg-max of a selecting Q row, the Huber branch -- is within those bounds: every element of every case is then compared on
the GPU, none is masked.
"""
import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
NAMES = ("w1", "b1", "w2", "b2", "w3", "b3")
LR, BETA1, BETA2, EPS = 1e-3, 0.9, 0.99, 1e-4          # the Adam settings of the GPU tests (DQNNet's defaults but lr)
DISCOUNT = 0.97


def make_weights(dims, A, rng, bias=0.1):
    """six fp32 tensors: Glorot-uniform kernels ([in][out]) like the networks' own initialisation, and biases that are
    NOT zero (a kernel that dropped or misplaced a bias would pass with the default zero biases)."""
    d0, h1, h2 = dims
    out = {}
    for k, (fi, fo) in zip(("1", "2", "3"), ((d0, h1), (h1, h2), (h2, A))):
        lim = np.sqrt(6.0 / (fi + fo))
        out["w" + k] = rng.uniform(-lim, lim, size=(fi, fo)).astype(F32)
        out["b" + k] = rng.uniform(-bias, bias, size=(fo,)).astype(F32)
    return out


def _dense(x, ex, w, b):
    """z = x w + b in float64 and the bound on an fp32 evaluation's distance from it; ex: the bound carried by x."""
    w, b = w.astype(F64), b.astype(F64)
    z = x @ w + b
    K = w.shape[0]
    with np.errstate(invalid="ignore"):
        bound = (K + 2) * U * (np.abs(x) @ np.abs(w) + np.abs(b)) + ex @ np.abs(w)
    return z, bound


def forward(W, x):
    """-> dict(z1, h1, z2, h2, q) in float64 and e1, e2, eq: the a-priori fp32 bounds of z1, z2, q."""
    x = np.asarray(x, dtype=F64)
    with np.errstate(invalid="ignore"):
        z1, e1 = _dense(x, np.zeros_like(x), W["w1"], W["b1"])
        h1 = np.maximum(z1, 0.0)
        z2, e2 = _dense(h1, e1, W["w2"], W["b2"])
        h2 = np.maximum(z2, 0.0)
        q, eq = _dense(h2, e2, W["w3"], W["b3"])
    return dict(z1=z1, h1=h1, z2=z2, h2=h2, q=q, e1=e1, e2=e2, eq=eq)


def update(W, Wt, s, s2, actions, rewards, game_overs, discount=DISCOUNT, iw=None, huber=False, ddqn=False):
    """One learn_from_batch up to the gradients.  W / Wt: online / target weights (dicts of NAMES, fp32).
    iw: importance weights (used as their fp32 values, like the fp32 placeholder they are fed to) or None.
    A row whose action is outside [0, A) raises status bit 1 and takes no part: no target, no |TD error| (NaN marks the
    untouched slot), no loss term, no gradient -- the mean still divides by B.
    -> q, q_next_target, q_next_online (None unless ddqn), selected, targets [B], td [B], e [B], loss, grads {name},
       norm, status, fwd / fwd_next_target / fwd_next_online (forward()'s dicts: all pre-activations and bounds)."""
    B = len(actions)
    A = W["b3"].shape[0]
    fo, ft = forward(W, s), forward(Wt, s2)
    fn = forward(W, s2) if ddqn else None
    sel_row = fn["q"] if ddqn else ft["q"]
    selected = np.argmax(sel_row, 1)                                        # first maximum, first NaN
    acts = np.asarray(actions).astype(np.int64)
    valid = (acts >= 0) & (acts < A)
    a_ok = np.where(valid, acts, 0)
    rows = np.arange(B)
    done = (np.asarray(game_overs) != 0).astype(F64)                        # any non-zero byte is terminal
    with np.errstate(invalid="ignore"):
        y = np.asarray(rewards, dtype=F64) + (1.0 - done) * float(discount) * ft["q"][rows, selected]
        qa = fo["q"][rows, a_ok]
        e = qa - y
        td = np.where(valid, np.abs(y - qa), np.nan)
        w = np.ones(B) if iw is None else np.asarray(iw).astype(F32).astype(F64)
        if huber:
            ae = np.abs(e)
            l = np.where(ae <= 1.0, 0.5 * e * e, ae - 0.5)
            g = np.where(np.isnan(e), np.nan, np.clip(e, -1.0, 1.0))
        else:
            l, g = e * e, 2.0 * e
        loss = np.sum(np.where(valid, w * l, 0.0)) / B
        dq = np.zeros((B, A))
        dq[rows[valid], a_ok[valid]] = (w * g / B)[valid]
        # backward: tf.gradients through three Dense layers
        grads = {}
        grads["w3"], grads["b3"] = fo["h2"].T @ dq, dq.sum(0)
        dz2 = (dq @ W["w3"].astype(F64).T) * (fo["h2"] > 0)
        grads["w2"], grads["b2"] = fo["h1"].T @ dz2, dz2.sum(0)
        dz1 = (dz2 @ W["w2"].astype(F64).T) * (fo["h1"] > 0)
        grads["w1"], grads["b1"] = np.asarray(s, dtype=F64).T @ dz1, dz1.sum(0)
        norm = np.sqrt(sum(float(np.sum(v * v)) for v in grads.values()))
    return dict(q=fo["q"], q_next_target=ft["q"], q_next_online=None if fn is None else fn["q"], selected=selected,
                targets=y, td=td, e=e, loss=loss, grads=grads, norm=norm, status=0 if valid.all() else 1,
                fwd=fo, fwd_next_target=ft, fwd_next_online=fn, valid=valid, taken=a_ok, dz2=dz2, dz1=dz1)


def adam_first_step(W, grads, lr=LR, beta1=BETA1, beta2=BETA2, eps=EPS):
    """TF1 Adam's first step from zero slots (optim.hip's adam_tf1_kernel, in float64) -> (weights, m, v)."""
    alpha = lr * np.sqrt(1.0 - beta2) / (1.0 - beta1)
    out, ms, vs = {}, {}, {}
    with np.errstate(invalid="ignore"):
        for k in NAMES:
            g = grads[k]
            ms[k], vs[k] = (1.0 - beta1) * g, (1.0 - beta2) * g * g
            out[k] = W[k].astype(F64) - alpha * ms[k] / (np.sqrt(vs[k]) + eps)
    return out, ms, vs


def ambiguity(res, huber, ddqn, discount=DISCOUNT):
    """How close a case's discontinuities sit to their a-priori fp32 bounds: the smallest ratio |distance| / bound over
    (a) every pre-activation of every tower the update evaluates (the sign decides relu and relu'), (b) the top-two gap
    of every selecting Q row against the two entries' bounds, (c) ||e| - 1| under Huber against the bound of e.
    A case is unambiguous when every ratio exceeds 1.  -> dict(z=, gap=, huber=) of the minima (inf where void)."""
    out = dict(z=np.inf, gap=np.inf, huber=np.inf)
    towers = [res["fwd"], res["fwd_next_target"]] + ([res["fwd_next_online"]] if ddqn else [])
    for f in towers:
        for z, b in ((f["z1"], f["e1"]), (f["z2"], f["e2"])):
            out["z"] = min(out["z"], float(np.min(np.abs(z) / b)))
    sel = towers[2] if ddqn else towers[1]
    q, eq = sel["q"], sel["eq"]
    finite = ~np.isnan(q).any(1)                    # (a row with a NaN selects its first NaN whatever the rounding)
    if q.shape[1] > 1 and finite.any():
        q, eq = q[finite], eq[finite]
        order = np.argsort(-q, axis=1)
        rows = np.arange(q.shape[0])
        first, second = order[:, 0], order[:, 1]
        gap = q[rows, first] - q[rows, second]
        out["gap"] = float(np.min(gap / (eq[rows, first] + eq[rows, second])))
    if huber:
        rows = np.arange(len(res["e"]))
        on_bound = res["fwd"]["eq"][rows, res["taken"]]
        tg_bound = res["fwd_next_target"]["eq"][rows, res["selected"]]
        # e = Q(s, a) - (float)y: the two Q values' bounds, the rounding of y to fp32 and of the difference
        be = on_bound + abs(discount) * tg_bound + U * np.abs(res["targets"]) + U * np.abs(res["e"])
        ratio = np.abs(np.abs(res["e"]) - 1.0) / be
        if not np.isnan(ratio).all():               # (a NaN error has no branch to miss)
            out["huber"] = float(np.nanmin(ratio))
    return out


# ------------------------------------------------------------------------------------------------------------------
# The seeded cases of tests/test_mlp_fused_edges.py.  (D0, H1, H2), A, B and the edge each shape is there for; G = H2 / 32
# workgroups, S1 = H1 / G columns of the first layer per workgroup.
SHAPES = [
    ((1, 32, 32), 1, 1),        # 0: smallest of everything; G = 1: the barrier target is 1
    ((16, 32, 32), 16, 32),     # 1: D0 = 16: all eight K steps of dense1; A = kMaxA: full qs rows, db3 lanes 64..79; full batch
    ((15, 32, 64), 16, 31),     # 2: odd D0 padded to 16; B = 31: one zero-padded row
    ((8, 288, 32), 3, 32),      # 3: largest H1 the LDS admits; nine column tiles (wave 0: 0, 4, 8, empty partner); G = 1, S1 = 288
    ((8, 288, 64), 2, 20),      # 4: S1 = 144 (dz1 staging beyond `red`)
    ((4, 256, 32), 2, 7),       # 5: S1 = 256
    ((4, 160, 32), 5, 32),      # 6: S1 = 160
    ((2, 288, 288), 4, 32),     # 7: G = 9: sum_strided runs its unrolled body once and leaves a remainder of 1
    ((4, 32, 1024), 2, 32),     # 8: G = 32, S1 = 1
    ((4, 64, 2048), 2, 32),     # 9: G = 64, the largest grid: eight unrolled rounds of sum_strided, no remainder
]
DDQN_SHAPES = (0, 3, 9)

# (shape index, huber, ddqn, importance weights: None | "f32" | "f64") -> seed, found by scanning seeds on the CPU for the
# first one whose case is unambiguous (tests/test_mlp_ref.py asserts that it is)
SEEDS = {
    (0, False, False, None): 1, (0, True, True, "f32"): 1, (0, False, True, "f64"): 1,
    (1, False, False, None): 1, (1, True, False, "f64"): 1,
    (2, False, False, None): 1, (2, True, False, "f32"): 1,
    (3, False, False, None): 2, (3, True, True, "f64"): 2, (3, False, True, "f32"): 2,
    (4, False, False, None): 2, (4, True, False, "f32"): 2,
    (5, False, False, None): 1, (5, True, False, "f64"): 1,
    (6, False, False, None): 1, (6, True, False, "f32"): 1,
    (7, False, False, None): 21, (7, True, False, "f64"): 21,
    (8, False, False, None): 1, (8, True, False, "f32"): 1,
    (9, False, False, None): 2, (9, True, True, "f64"): 2, (9, False, True, "f32"): 2,
}


def case_list():
    """every shape with MSE (DQN, no importance weights) and with Huber (Double DQN on DDQN_SHAPES, importance weights
    given as fp32 on even shapes and as fp64 on odd ones); DDQN_SHAPES also with MSE + Double DQN + weights"""
    out = []
    for i in range(len(SHAPES)):
        out.append((i, False, False, None))
        out.append((i, True, i in DDQN_SHAPES, "f32" if i % 2 == 0 else "f64"))
        if i in DDQN_SHAPES:
            out.append((i, False, True, "f64" if i % 2 == 0 else "f32"))
    return out


def make_case(key, seed=None):
    """-> dict(dims, A, B, huber, ddqn, W, Wt, s, s2, a, r, done, iw (fp32 values or None), iw_kind).  The target network's
    weights are a draw of their own (a kernel that read the online copy for the target tower would pass otherwise).
    Importance weights: one of them exactly 0 where B > 1 (at B = 1 a zero weight would zero every gradient)."""
    i, huber, ddqn, iw_kind = key
    dims, A, B = SHAPES[i]
    rng = np.random.RandomState(SEEDS[key] if seed is None else seed)
    W, Wt = make_weights(dims, A, rng), make_weights(dims, A, rng)
    s = rng.randn(B, dims[0]).astype(F32)
    s2 = rng.randn(B, dims[0]).astype(F32)
    a = rng.randint(0, A, B).astype(np.int32)
    r = rng.randn(B).astype(F32)
    done = (rng.rand(B) < 0.2).astype(np.uint8)
    iw = None
    if iw_kind is not None:
        iw = (rng.rand(B) + 0.1).astype(F32)
        if B > 1:
            iw[B // 2] = 0.0
    return dict(key=key, dims=dims, A=A, B=B, huber=huber, ddqn=ddqn, W=W, Wt=Wt, s=s, s2=s2, a=a, r=r, done=done, iw=iw,
                iw_kind=iw_kind)


PARAM_NAMES = dict(w1="main/embedder/dense0/kernel", b1="main/embedder/dense0/bias", w2="main/middleware/dense0/kernel",
                   b2="main/middleware/dense0/bias", w3="main/q_head/dense/kernel", b3="main/q_head/dense/bias")

EDGE_SHAPE = ((8, 96, 96), 5, 20)      # the semantic edges' shape: three workgroups, a ragged batch
NAN_SEEDS = {False: 1, True: 2}       # ddqn -> seed (scanned on the CPU like SEEDS)


def make_nan_case(ddqn, seed=None):
    """EDGE_SHAPE, MSE, a NaN in element 1 of the TARGET network's last bias: Q_target(s', 1) is NaN in every row.
    DQN: np.argmax selects the NaN in every row; Double DQN: in the rows whose online Q(s') peaks at column 1.  (MSE: its
    gradient 2 e is NaN for a NaN error on the device and in numpy alike.  Under Huber the kernels' clamp of a NaN error
    gives -1 where np.clip gives NaN -- DESIGN.md section 6 leaves that element open -- so no NaN reaches the backward
    pass on the device and there is nothing to compare.)  States
    are |N(0, 1)| draws: with non-negative inputs some units of both hidden layers are inactive over the whole batch,
    which is where `h > 0 ? dy : 0` and `dy * (h > 0)` part ways (tests/test_mlp_ref.py asserts that there are some)."""
    dims, A, B = EDGE_SHAPE
    rng = np.random.RandomState(NAN_SEEDS[ddqn] if seed is None else seed)
    W, Wt = make_weights(dims, A, rng), make_weights(dims, A, rng)
    Wt["b3"][1] = np.nan
    s = np.abs(rng.randn(B, dims[0])).astype(F32)
    s2 = np.abs(rng.randn(B, dims[0])).astype(F32)
    a = rng.randint(0, A, B).astype(np.int32)
    r = rng.randn(B).astype(F32)
    done = (rng.rand(B) < 0.2).astype(np.uint8)
    return dict(key=("nan", ddqn), dims=dims, A=A, B=B, huber=False, ddqn=ddqn, W=W, Wt=Wt, s=s, s2=s2, a=a, r=r, done=done,
                iw=None, iw_kind=None)


EDGE_VARIANTS = ("all_done", "done_255", "discount_0", "bad_actions")
EDGE_SEED = 5
BAD_ROWS = (3, 11)                     # "bad_actions": row 3 takes action -1, row 11 action A


def make_edge_case(variant, ddqn=False):
    """the semantic edges at EDGE_SHAPE (Huber, fp64 importance weights): every game_over = 1 (targets = rewards); one
    game_over byte of 255 (terminal like 1); discount = 0; two refused actions.  -> (case dict, discount)"""
    dims, A, B = EDGE_SHAPE
    rng = np.random.RandomState(EDGE_SEED)
    W, Wt = make_weights(dims, A, rng), make_weights(dims, A, rng)
    s = rng.randn(B, dims[0]).astype(F32)
    s2 = rng.randn(B, dims[0]).astype(F32)
    a = rng.randint(0, A, B).astype(np.int32)
    r = rng.randn(B).astype(F32)
    done = (rng.rand(B) < 0.2).astype(np.uint8)
    iw = (rng.rand(B) + 0.1).astype(F32)
    discount = DISCOUNT
    if variant == "all_done":
        done[:] = 1
    elif variant == "done_255":
        done[:] = 0
        done[7] = 255
    elif variant == "discount_0":
        discount = 0.0
    elif variant == "bad_actions":
        a[BAD_ROWS[0]], a[BAD_ROWS[1]] = -1, A
    else:
        raise ValueError(variant)
    return dict(key=(variant, ddqn), dims=dims, A=A, B=B, huber=True, ddqn=ddqn, W=W, Wt=Wt, s=s, s2=s2, a=a, r=r,
                done=done, iw=iw, iw_kind="f64"), discount


def make_huber_one_case(sign):
    """Huber at |e| = 1 exactly: every weight 0, b3 = sign / 2, r = -sign / 2, every row terminal -> Q = sign / 2 and
    y = -sign / 2 without rounding, e = sign.  Both branches give the loss 0.5 per row; the gradient is sign * iw / B at
    the taken action -- only b3 has a gradient (h1 = h2 = relu(0) = 0)."""
    dims, A, B = EDGE_SHAPE
    rng = np.random.RandomState(EDGE_SEED)
    W = {k: np.zeros((fi, fo) if k[0] == "w" else (fo,), dtype=F32)
         for k, (fi, fo) in zip(NAMES, ((dims[0], dims[1]),) * 2 + ((dims[1], dims[2]),) * 2 + ((dims[2], A),) * 2)}
    W["b3"][:] = 0.5 * sign
    s = rng.randn(B, dims[0]).astype(F32)
    s2 = rng.randn(B, dims[0]).astype(F32)
    a = rng.randint(0, A, B).astype(np.int32)
    r = np.full(B, -0.5 * sign, dtype=F32)
    done = np.ones(B, dtype=np.uint8)
    iw = (rng.randint(1, 9, B) / 8.0).astype(F32)          # exact in fp32, and so are their sums
    return dict(key=("huber_one", sign), dims=dims, A=A, B=B, huber=True, ddqn=False, W=W, Wt={k: v.copy() for k, v in W.items()},
                s=s, s2=s2, a=a, r=r, done=done, iw=iw, iw_kind="f64")


def inactive_units(res):
    """-> (units of h1, units of h2) that are inactive in every row of the batch beyond their fp32 bounds"""
    f = res["fwd"]
    return (np.flatnonzero((f["z1"] < -f["e1"]).all(0)), np.flatnonzero((f["z2"] < -f["e2"]).all(0)))


def run_case(c, discount=DISCOUNT):
    return update(c["W"], c["Wt"], c["s"], c["s2"], c["a"], c["r"], c["done"], discount, c["iw"], c["huber"], c["ddqn"])
