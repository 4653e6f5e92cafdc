"""Normalized Advantage Functions: numpy restatement of the head, its loss and its gradient — the arithmetic that
rlx_naf_head_loss / rlx_naf_head_forward (csrc/naf.hip) reproduce operation for operation.

Reference (paths under rl_coach/): architectures/tensorflow_components/heads/naf_head.py:45-86 (the head),
agents/naf_agent.py:83-90 (TD targets), heads/head.py:143-186 (the loss: tf.losses.mean_squared_error, or huber_loss
with delta 1 when replace_mse_with_huber_loss is set; mean over the batch, no importance weights).

Packing (naf_head.py:63-73): column c of the lower-triangular L occupies l_vector[i_c : i_c + A - c] with
i_c = sum_{k<c} (A - k);  L[c][c] = exp(l[i_c]),  L[r][c] = l[i_c + r - c] for r > c,  0 for r < c.

The order of operations, which is THE PROJECT'S DEFINITION of the head: TensorFlow forms P = L L^T first and its
op-level rounding is unpinned, so nothing finer than fp32 rounding error can be taken from it.
Everything is fp32 unless stated, every sum runs in ascending index order starting from the first term, and no
multiply-add is contracted:
    mu_c   = mu_unscaled_c * output_scale_c            (mu_unscaled is the Dense layer's activated output)
    d_c    = u_c - mu_c
    y_c    = sum_{r = c .. A-1} L[r][c] * d_r          (y = L^T d)
    Adv    = -0.5 * sum_c y_c * y_c
    Q      = V + Adv
    target = fp32( fp64(r) + (1 - game_over) * discount * fp64(V_target(s')) )     (rlx_dqn_head_loss's rounding point)
    e      = Q - target;   mean squared: term = e * e, dterm = 2 e;   Huber: term = 0.5 e e if |e| <= 1 else |e| - 0.5,
                           dterm = clip(e, -1, 1)
    loss   = tree_sum(term) / B                        (pairwise tree over 256 leaves, rows beyond the batch are zero)
    g      = grad_scale * dterm / B                    (= d loss / d Q of the row)
    dV     = g
    (L y)_c = sum_{k = 0 .. c} L[c][k] * y_k
    dmu_unscaled_c = (g * (L y)_c) * output_scale_c
    t_c    = -g * y_c;   dL[r][c] = t_c * d_r  (r >= c)
    dl[i_c] = dL[c][c] * L[c][c];   dl[i_c + r - c] = dL[r][c]  (r > c)
"""
import numpy as np

F32 = np.float32
TREE_LEAVES = 256


def column_starts(A):
    """i_c of every column: [0, A, 2A - 1, ...]."""
    out, i = [], 0
    for c in range(A):
        out.append(i)
        i += A - c
    return out


def packed_size(A):
    return A * (A + 1) // 2


def build_L(l_vector, A):
    """[B, A(A+1)/2] -> L [B, A, A] fp32 (lower triangular, exponentiated diagonal)."""
    l = np.asarray(l_vector, dtype=F32)
    B = l.shape[0]
    L = np.zeros((B, A, A), dtype=F32)
    for c, i in enumerate(column_starts(A)):
        L[:, c, c] = np.exp(l[:, i])
        for r in range(c + 1, A):
            L[:, r, c] = l[:, i + r - c]
    return L


def forward(v, mu_unscaled, l_vector, output_scale, actions=None):
    """-> dict(mu [B,A], d, L [B,A,A], y, adv [B], q [B]); actions None: u = mu (Adv = 0, Q = V)."""
    v = np.asarray(v, dtype=F32).reshape(-1)
    mu_u = np.asarray(mu_unscaled, dtype=F32)
    B, A = mu_u.shape
    scale = np.broadcast_to(np.asarray(output_scale, dtype=F32), (A,))
    mu = (mu_u * scale).astype(F32)
    L = build_L(l_vector, A)
    d = np.zeros((B, A), dtype=F32) if actions is None else (np.asarray(actions, dtype=F32) - mu).astype(F32)
    y = np.zeros((B, A), dtype=F32)
    for c in range(A):
        s = (L[:, c, c] * d[:, c]).astype(F32)
        for r in range(c + 1, A):
            s = (s + (L[:, r, c] * d[:, r]).astype(F32)).astype(F32)
        y[:, c] = s
    ss = (y[:, 0] * y[:, 0]).astype(F32)
    for c in range(1, A):
        ss = (ss + (y[:, c] * y[:, c]).astype(F32)).astype(F32)
    adv = (F32(-0.5) * ss).astype(F32)
    if actions is None:
        adv = np.zeros(B, dtype=F32)
    q = (v + adv).astype(F32)
    return dict(mu=mu, d=d, L=L, y=y, adv=adv, q=q)


def td_targets(rewards, game_overs, discount, v_next):
    """naf_agent.py:89-90 in fp64 (numpy promotes), rounded to fp32 where the network's placeholder takes it."""
    r = np.asarray(rewards, dtype=F32).astype(np.float64)
    go = np.asarray(game_overs).astype(bool).astype(np.float64)
    vn = np.asarray(v_next, dtype=F32).reshape(-1).astype(np.float64)
    return (r + (1.0 - go) * float(discount) * vn).astype(F32)


def tree_sum(terms):
    red = np.zeros(TREE_LEAVES, dtype=F32)
    red[:len(terms)] = terms
    d = TREE_LEAVES >> 1
    while d > 0:
        red[:d] = (red[:d] + red[d:2 * d]).astype(F32)
        d >>= 1
    return red[0]


def update(v, mu_unscaled, l_vector, output_scale, actions, v_next, rewards, game_overs, discount, huber=False,
           grad_scale=1.0):
    """The head's loss and gradient -> dict(loss, dv [B], dmu_unscaled [B,A], dl [B,A(A+1)/2], td_targets, q, adv,
    mu, L)."""
    f = forward(v, mu_unscaled, l_vector, output_scale, actions)
    L, d, y, q = f["L"], f["d"], f["y"], f["q"]
    B, A = d.shape
    assert 1 <= B <= TREE_LEAVES
    scale = np.broadcast_to(np.asarray(output_scale, dtype=F32), (A,))
    tgt = td_targets(rewards, game_overs, discount, v_next)
    e = (q - tgt).astype(F32)
    if huber:
        ae = np.abs(e)
        term = np.where(ae <= F32(1), (F32(0.5) * e * e).astype(F32), (ae - F32(0.5)).astype(F32)).astype(F32)
        dterm = np.clip(e, F32(-1), F32(1)).astype(F32)
    else:
        term = (e * e).astype(F32)
        dterm = (F32(2) * e).astype(F32)
    loss = F32(tree_sum(term) / F32(B))
    g = ((F32(grad_scale) * dterm).astype(F32) / F32(B)).astype(F32)
    dmu_u = np.zeros((B, A), dtype=F32)
    for c in range(A):
        s = (L[:, c, 0] * y[:, 0]).astype(F32)
        for k in range(1, c + 1):
            s = (s + (L[:, c, k] * y[:, k]).astype(F32)).astype(F32)
        dmu_u[:, c] = ((g * s).astype(F32) * scale[c]).astype(F32)
    dl = np.zeros((B, packed_size(A)), dtype=F32)
    for c, i in enumerate(column_starts(A)):
        t = ((-g).astype(F32) * y[:, c]).astype(F32)
        dl[:, i] = ((t * d[:, c]).astype(F32) * L[:, c, c]).astype(F32)
        for r in range(c + 1, A):
            dl[:, i + r - c] = (t * d[:, r]).astype(F32)
    return dict(loss=loss, dv=g, dmu_unscaled=dmu_u, dl=dl, td_targets=tgt, q=q, adv=f["adv"], mu=f["mu"], L=L)
