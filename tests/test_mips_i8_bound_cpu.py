"""CPU: soundness of the int8 filter of csrc/mips_scan8i.hip, on the numpy restatement tools/mips_i8_filter_study.py keeps of its
quantisation, block constants and integer threshold.  Against float64 scores of the fp16 operands (exact products, 768-term sums: error
~1e-13 relative) and exact integer sums:

  * |S - t_q s_b I| <= eps(q, b) for EVERY (query, row) pair,
  * for tau at several quantiles of a query's scores (and the extremes), no row with S >= tau has I < Theta(q, b).

Conditions, not measurements: zero violations."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("mips_i8_filter_study", os.path.join(ROOT, "tools", "mips_i8_filter_study.py"))
st = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(st)


def _normal(rng, n, dim):
    return rng.standard_normal((n, dim)).astype(np.float16)


def _clustered(rng, n, dim):
    """The clustered generator's shape: 32-row topics (cosine 0.64 to the topic centre), log-normal topic norms (sigma 0.25)."""
    nt = (n + 31) // 32
    centers = rng.standard_normal((nt, dim))
    scales = np.exp(0.25 * rng.standard_normal(nt))
    x = 0.6 * rng.standard_normal((nt, 32, dim)) + 0.8 * centers[:, None, :]
    return (x * scales[:, None, None]).reshape(nt * 32, dim)[:n].astype(np.float16)


def _ternary(rng, n, dim):
    return rng.integers(-1, 2, size=(n, dim)).astype(np.float16)


def _mixed_magnitudes(rng, n, dim):
    """Every block mixes one row of magnitude 6e4 (near the fp16 maximum) with tiny rows: the block scale is set by the huge row and the
    tiny rows quantise to zero -- their whole norm lands in D_b."""
    x = (1e-3 * rng.standard_normal((n, dim))).astype(np.float16)
    x[::256] = (6.0e4 * np.sign(rng.standard_normal((len(x[::256]), dim)))).astype(np.float16)
    x[5::256] = (30.0 * rng.standard_normal((len(x[5::256]), dim))).astype(np.float16)
    return x


def _zero_blocks(rng, n, dim):
    x = _normal(rng, n, dim)
    x[256:512] = 0                                                   # an all-zero block: s_b = 0, "everything survives", eps = 0
    x[1024:1100] = 0
    return x


def _subnormals(rng, n, dim):
    x = (rng.integers(-1023, 1024, size=(n, dim)).astype(np.float64) * 2.0 ** -24).astype(np.float16)       # every value an fp16 subnormal
    x[300:400] = _normal(rng, 100, dim)
    return x


CORPORA = {"normal": _normal, "clustered": _clustered, "ternary": _ternary, "mixed_magnitudes": _mixed_magnitudes, "zero_blocks": _zero_blocks,
           "subnormals": _subnormals}


def _queries(rng, rows, nq, dim):
    q = rng.standard_normal((nq, dim)).astype(np.float16)
    q[1] = rows[-7]                                                  # a query that IS a late row
    q[2] = (rows[-40].astype(np.float64) * 0.5 + 0.3 * rng.standard_normal(dim)).astype(np.float16)
    q[3] = 0                                                         # the zero query: t_q = 0
    q[4] = (q[4].astype(np.float64) * 2.0 ** -14).astype(np.float16)  # a tiny query (subnormal entries)
    q[5] = (200.0 * rng.standard_normal(dim)).astype(np.float16)      # a large one
    return q


@pytest.mark.parametrize("dim", [256, 768])
@pytest.mark.parametrize("corpus", sorted(CORPORA))
def test_bound_holds_and_nothing_above_tau_is_pruned(corpus, dim):
    rng = np.random.default_rng(sorted(CORPORA).index(corpus) * 1000 + dim)
    n, nq = 2000, 12                                                 # 8 blocks, the last one short
    rows = CORPORA[corpus](rng, n, dim)
    assert np.isfinite(rows.astype(np.float32)).all()
    queries = _queries(rng, rows, nq, dim)
    e8, blk = st.quantise_blocks(rows)
    q8, qc = st.quantise_queries(queries)
    assert np.abs(e8.astype(np.int32)).max() <= 127 and np.abs(q8.astype(np.int32)).max() <= 127
    I = st.int_scores(e8, q8)
    assert np.abs(I).max() <= dim * 127 * 127
    S = queries.astype(np.float64) @ rows.astype(np.float64).T
    blk_of = np.arange(n) // st.BLOCK

    # (1) the bound, every pair
    approx = qc[:, 0:1].astype(np.float64) * blk[blk_of, 0].astype(np.float64)[None, :] * I
    eps = st.epsilon(qc, blk).astype(np.float64)[:, blk_of]
    viol = np.abs(S - approx) > eps
    assert int(viol.sum()) == 0, "|S - t s I| > eps for %d pairs (worst excess %.3g)" % (viol.sum(), (np.abs(S - approx) - eps).max())

    # (2) the integer threshold never prunes a row at or above tau
    taus = [np.quantile(S, ql, axis=1) for ql in (0.0, 0.5, 0.9, 0.97, 0.999, 1.0)]
    taus += [np.full(nq, -np.inf), np.zeros(nq), S.max(axis=1) + 1.0]
    for tau in taus:
        tau32 = tau.astype(np.float32)                               # the kernel holds tau as float32
        th = st.theta(tau32, qc, blk)[:, blk_of]
        pruned_wrongly = (S >= tau32[:, None].astype(np.float64)) & (I < th)
        assert int(pruned_wrongly.sum()) == 0, "%d rows with S >= tau pruned" % pruned_wrongly.sum()
    # tau = +inf (a padded query column) prunes everything; a zero scale prunes nothing
    th = st.theta(np.full(nq, np.inf, dtype=np.float32), qc, blk)
    assert (th == (1 << 31) - 1).all()
    th = st.theta(np.zeros(nq, dtype=np.float32), qc, blk)
    assert (th[3] == -(1 << 31)).all()                               # the zero query
    if corpus == "zero_blocks":
        assert blk[1, 0] == 0 and (th[:, 1] == -(1 << 31)).all() and (e8[256:512] == 0).all()


def test_filter_is_selective_on_normal_data():
    """Not a soundness condition: the bound is tight enough to be a filter at all (eps well below the score spread, survivors a small
    multiple of the fp16 filter's) -- the figures of profiles/mips_i8_filter_study.txt at a size a test can afford."""
    rng = np.random.default_rng(5)
    n, nq, dim = 40000, 4, 768
    rows, queries = _normal(rng, n, dim), _normal(rng, nq, dim)
    e8, blk = st.quantise_blocks(rows)
    q8, qc = st.quantise_queries(queries)
    I = st.int_scores(e8, q8)
    S = queries.astype(np.float64) @ rows.astype(np.float64).T
    assert st.epsilon(qc, blk).max() < S.std()
    tau = np.sort(S, axis=1)[:, -64].astype(np.float32)
    th = st.theta(tau, qc, blk)[:, np.arange(n) // st.BLOCK]
    survivors = (I >= th).sum(axis=1)
    assert (survivors >= 64).all() and survivors.max() < 64 * 20
