"""CPU: soundness of the deferred drop of csrc/mips_scan8i.hip.  A survivor of an int8 segment that is not re-scored at
once waits under  U(q, b, I) = t_q s_b I + eps(q, b) + slack(q, b)  and is dropped unread once U < tau.  On the numpy restatement
tools/mips_i8_filter_study.py keeps of the quantisation and the block / query constants, with U restated here operation by operation in
float32 (s8i_upper) and everything it is compared with in float64:

  * |S - t_q s_b I| <= eps(q, b) for EVERY (query, row) pair, on the families of the GPU test and on rows whose quantisation residual is
    aligned with the query, where the observed error comes close to eps,
  * U < tau implies S < tau for the exact score S and S32 < tau for the fp32-accumulated score S32 of the re-score (exact fp16 products
    summed in float32 in the order of rescore_wave_x4), for tau at quantiles of a query's scores and at S itself (the tightest tau a row
    meets) -- and U >= S32 outright,
  * the slack covers the model: an n-term float32 sum of exact products is off by at most n 2^-24 / (1 - n 2^-24) * sum |q_i e_i|
    <= that * ||q|| ||e|| (Higham, Accuracy and Stability of Numerical Algorithms, 4.4 -- any order), and ||q|| <= a_q + b_q, ||e|| <= N_b.

Conditions, not measurements: zero violations."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("mips_i8_filter_study", os.path.join(ROOT, "tools", "mips_i8_filter_study.py"))
st = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(st)
F = np.float32


def upper(I, qc, blk, blk_of, dim):
    """s8i_upper in float32, [Q, N]: (est, eps, U)"""
    t, a, b = (qc[:, j:j + 1].astype(F) for j in range(3))
    s, n, d = (blk[blk_of, j][None, :].astype(F) for j in range(3))
    est = (t * s) * I.astype(F)
    eps = (a * n + b * d) * F(1.0001)
    slack = F(dim) * F(2.0 ** -22) * (a + b) * n * F(1.0001)
    u = est + np.abs(est) * F(1e-6) + eps + slack
    return est, eps, u + np.abs(u) * F(1e-6)


def rescore_f32(rows, queries):
    """The fp32 sum of rescore_wave_x4, [Q, N]: lane l adds the products of its 8-element segments l, l + 64, .. one after the other, then
    the xor tree over the 64 lanes."""
    n, dim = rows.shape
    nseg = dim // 8
    p = queries.astype(F)[:, None, :] * rows.astype(F)[None, :, :]       # exact: 11 x 11 significant bits
    p = p.reshape(len(queries), n, nseg, 8)
    lane = np.zeros((len(queries), n, 64), dtype=F)
    for it in range((nseg + 63) // 64):
        segs = np.arange(64) + 64 * it
        ok = segs < nseg
        for j in range(8):
            add = np.zeros_like(lane)
            add[:, :, ok] = p[:, :, segs[ok], j]
            lane = (lane + add).astype(F)
    for o in (32, 16, 8, 4, 2, 1):
        lane = (lane + lane[:, :, np.arange(64) ^ o]).astype(F)
    return lane[:, :, 0]


def _u(rng, dim):
    u = rng.standard_normal(dim)
    return u / np.linalg.norm(u)


def _winners(rng, n, dim, late):
    u = _u(rng, dim)
    rows = (0.05 * rng.standard_normal((n, dim))).astype(np.float16)
    at = (n - 1 - rng.permutation(n // 50)[:20]) if late else rng.permutation(n // 50)[:20]
    rows[at] = ((1.0 + rng.random((20, 1))) * u[None, :] + 0.01 * rng.standard_normal((20, dim))).astype(np.float16)
    return rows, (u[None, :] + 0.05 * rng.standard_normal((12, dim))).astype(np.float16)


def late_winners(rng, n, dim):
    return _winners(rng, n, dim, True)


def early_winners(rng, n, dim):
    return _winners(rng, n, dim, False)


def outlier_blocks(rng, n, dim):
    u = _u(rng, dim)
    rows = (0.05 * rng.standard_normal((n, dim))).astype(np.float16)
    at = np.arange(17, n, 256)
    x = 5.0 * rng.standard_normal((len(at), dim))
    rows[at] = (x - (x @ u)[:, None] * u[None, :] - 40.0 * u[None, :]).astype(np.float16)
    win = rng.permutation(n)[:60]
    win = win[(win % 256) != 17]
    rows[win] = ((6.0 + 4.0 * rng.random((len(win), 1))) * u[None, :] + 0.01 * rng.standard_normal((len(win), dim))).astype(np.float16)
    return rows, (u[None, :] + 0.02 * rng.standard_normal((12, dim))).astype(np.float16)


def crowded_band(rng, n, dim):
    u = _u(rng, dim)
    rows = (0.02 * rng.standard_normal((n, dim))).astype(np.float16)
    rows[:64] = (np.linspace(1.6, 2.0, 64)[:, None] * u[None, :] + 0.0005 * rng.standard_normal((64, dim))).astype(np.float16)
    band = 64 + rng.permutation(n - 64)[:n // 3]
    c = 1.597 - 0.023 * rng.random((len(band), 1))
    rows[band] = (c * u[None, :] + 0.0005 * rng.standard_normal((len(band), dim))).astype(np.float16)
    return rows, (u[None, :] + 0.0005 * rng.standard_normal((12, dim))).astype(np.float16)


def degenerate_constants(rng, n, dim):
    rows = rng.standard_normal((n, dim)).astype(np.float16)
    rows[256:512] = 0
    q = rng.standard_normal((12, dim)).astype(np.float16)
    q[3] = 0
    q[4] = rows[700]
    q[5] = rows[n - 5]
    q[6] = (q[6].astype(np.float64) * 2.0 ** -12).astype(np.float16)
    q[7] = (q[7].astype(np.float64) * 100.0).astype(np.float16)
    return rows, q


def duplicates(rng, n, dim):
    rows = rng.standard_normal((n, dim)).astype(np.float16)
    rows[rng.integers(0, n, n // 4)] = rows[rng.integers(0, n, n // 4)]
    return rows, rng.standard_normal((12, dim)).astype(np.float16)


def aligned_residual(rng, n, dim):
    """Rows whose quantisation residual is a fixed fraction of a step in the direction of the query's signs, against queries that quantise
    exactly (every element +-c: a_q ~ 0): q.(e - s e8) = t s 0.4375 * 127 dim = b_q D_b.  Block scale s = 1 / 8 (one element is 127 / 8), row
    elements (k + 0.4375 sgn_i) / 8 with |k| <= 100: multiples of 2^-7 below 16, exact in fp16.  Two sign patterns, for two of the queries;
    the other queries see the same rows at an angle."""
    sg = np.where(rng.standard_normal((2, dim)) > 0, 1.0, -1.0)
    k = rng.integers(-100, 101, size=(n, dim)).astype(np.float64)
    rows = (k + 0.4375 * sg[(np.arange(n) // 256) % 2][:, :]) / 8.0
    rows[::256, 0] = 127.0 / 8.0
    rows = rows.astype(np.float16)
    assert np.array_equal(rows.astype(np.float64)[1], ((k + 0.4375 * sg[0]) / 8.0)[1])
    q = rng.standard_normal((12, dim)).astype(np.float16)
    q[0] = (0.75 * sg[0]).astype(np.float16)
    q[1] = (3.0 * sg[1]).astype(np.float16)
    q[2] = (-0.75 * sg[0]).astype(np.float16)
    return rows, q


FAMILIES = {f.__name__: f for f in (late_winners, early_winners, outlier_blocks, crowded_band, degenerate_constants, duplicates, aligned_residual)}


@pytest.mark.parametrize("dim", [256, 768])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_a_deferred_drop_never_drops_a_row_at_or_above_tau(family, dim):
    rng = np.random.default_rng(sorted(FAMILIES).index(family) * 1000 + dim)
    n = 1500                                                             # 6 blocks, the last one short
    rows, queries = FAMILIES[family](rng, n, dim)
    assert np.isfinite(rows.astype(np.float32)).all()
    nq = len(queries)
    e8, blk = st.quantise_blocks(rows)
    q8, qc = st.quantise_queries(queries)
    I = st.int_scores(e8, q8)
    blk_of = np.arange(n) // st.BLOCK
    S = queries.astype(np.float64) @ rows.astype(np.float64).T
    S32 = rescore_f32(rows, queries)
    est, eps, U = upper(I, qc, blk, blk_of, dim)

    # (1) the bound, every pair, in float64 on the float32 constants
    approx = qc[:, 0:1].astype(np.float64) * blk[blk_of, 0].astype(np.float64)[None, :] * I
    eps64 = st.epsilon(qc, blk).astype(np.float64)[:, blk_of]
    err = np.abs(S - approx)
    assert int((err > eps64).sum()) == 0, "|S - t s I| > eps for %d pairs" % (err > eps64).sum()
    assert np.array_equal(eps.astype(np.float64), eps64)                 # the restatement above forms the study's eps
    if family == "aligned_residual":
        ratio = err[:2] / eps64[:2]
        assert ratio.max() > 0.9, "the aligned rows reach only %.3f of eps" % ratio.max()

    # (2) the slack covers the model of an n-term float32 sum, and U is above both scores outright
    qn = np.linalg.norm(queries.astype(np.float64), axis=1)[:, None]
    en = np.linalg.norm(rows.astype(np.float64), axis=1)[None, :]
    gamma = dim * 2.0 ** -24 / (1.0 - dim * 2.0 ** -24)
    assert (np.abs(S32.astype(np.float64) - S) <= gamma * qn * en).all()
    U64 = U.astype(np.float64)
    assert (U64 - (approx + eps64) >= gamma * qn * en).all(), "the slack in U is below the model's accumulation error"
    assert (U64 >= S).all() and (U64 >= S32.astype(np.float64)).all()

    # (3) the drop rule: U < tau implies S < tau and S32 < tau
    taus = [np.quantile(S, ql, axis=1) for ql in (0.0, 0.5, 0.9, 0.97, 0.999, 1.0)]
    taus += [np.full(nq, -np.inf), np.zeros(nq), S.max(axis=1) + 1.0]
    for tau in taus:
        tau32 = tau.astype(F)                                            # the kernels hold tau as float32
        dropped = U < tau32[:, None]
        t64 = tau32.astype(np.float64)[:, None]
        assert int((dropped & (S >= t64)).sum()) == 0 and int((dropped & (S32 >= tau32[:, None])).sum()) == 0
    # ... and with every row's own fp32 score as tau: the tightest threshold under which the row must still be kept
    assert not (U < S32).any()
    # the zero query and the all-zero block: estimate 0, bound 0, score 0
    if family == "degenerate_constants":
        assert (U[3] == 0).all() and (S[3] == 0).all()
        assert (est[:, 256:512] == 0).all() and (U[:, 256:512] == 0).all() and (S[:, 256:512] == 0).all()


def test_most_deferred_rows_die_on_normal_data():
    """Not a soundness condition: on N(0,1) data the bound is tight enough to pay -- once tau has risen by 0.7 sigma of the score distribution
    (what it does between the first int8 segment and the end of the flagship index), most of a segment's deferred survivors have U < tau."""
    rng = np.random.default_rng(11)
    n, nq, dim = 40000, 4, 768
    rows = rng.standard_normal((n, dim)).astype(np.float16)
    queries = rng.standard_normal((nq, dim)).astype(np.float16)
    e8, blk = st.quantise_blocks(rows)
    q8, qc = st.quantise_queries(queries)
    I = st.int_scores(e8, q8)
    blk_of = np.arange(n) // st.BLOCK
    S = queries.astype(np.float64) @ rows.astype(np.float64).T
    est, eps, U = upper(I, qc, blk, blk_of, dim)
    tau = np.sort(S, axis=1)[:, -64].astype(F)
    th = st.theta(tau, qc, blk)[:, blk_of]
    deferred = (I >= th) & ~(est + F(0.25) * eps >= tau[:, None])
    later = (tau + F(0.7) * S.std(axis=1).astype(F))[:, None]
    assert deferred.sum() > 0 and (deferred & (U < later)).sum() > 0.9 * deferred.sum()
