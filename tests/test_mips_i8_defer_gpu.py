"""GPU: the deferred re-score of the int8 segments (csrc/mips_scan8i.hip triage_kernel / rescore_pending_kernel) changes
no result.  A survivor of an int8 segment is either re-scored at once (its integer estimate reaches tau) or parked under an upper bound U and
read at the end of the search only if U still reaches the final tau.  Every case compares a shard with a shadow image with the same shard
fp16-only on search, search_f32 and search_records, fast path alone (exact_fallback=False, flags included), bit for bit, and five sampled
queries with the all-exact integer path.

Every case: 130 queries (one 256-query half, padded column tiles) and 512, k in {1, 50, 120} (kp = 64 and 128), a row count that is no multiple
of 256, row_base != 0, permuted ids.  At 290,003 rows of dimension 256 and a 16,384-row int8 threshold the schedule is a dense segment of
8,192 rows, then [8,192, 65,536), [65,536, 131,072), [131,072, end): the last two run on the int8 image at 130 queries, all three at 512.

Families (what each forces is in its generator's docstring).  Sizes are chosen so that the fp16-only shard raises no overflow flag -- asserted:
a case that only tests the fallback tests nothing new."""
import pytest
import torch

from tests.test_mips_i8_gpu import MIN_ROWS, _assert_same, _launches, _pair

pytestmark = pytest.mark.gpu

N, DIM, BASE = 290_003, 256, 77_001
NQ_MAX = 512


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _unit(g):
    u = torch.randn(DIM, generator=g, device="cuda", dtype=torch.float64)
    return u / u.norm()


def _near(u, g, noise):
    """NQ_MAX queries close to the direction u"""
    return (u[None, :] + noise * torch.randn((NQ_MAX, DIM), generator=g, device="cuda", dtype=torch.float64)).to(torch.float16)


def _planted(u, g, m, lo, hi):
    """m rows along u with scores in [lo, hi) against a query near u"""
    c = lo + (hi - lo) * torch.rand((m, 1), generator=g, device="cuda", dtype=torch.float64)
    return (c * u[None, :] + 0.01 * torch.randn((m, DIM), generator=g, device="cuda", dtype=torch.float64)).to(torch.float16)


def late_winners():
    """400 winners planted in the last 2 % of the rows, far above everything before: tau jumps at the very end, every pending entry of the
    earlier segments must die unread and the winners themselves arrive in the last triage."""
    g = _gen(1)
    u = _unit(g)
    rows = (0.05 * torch.randn((N, DIM), generator=g, device="cuda")).to(torch.float16)
    at = N - 1 - torch.randperm(N // 50, generator=g, device="cuda")[:400]
    rows[at] = _planted(u, g, 400, 1.0, 2.0)
    return rows, _near(u, g, 0.05)


def early_winners():
    """The reverse: the winners sit in the dense segment, tau is final before the first int8 segment: little triage work, nothing to re-score."""
    g = _gen(2)
    u = _unit(g)
    rows = (0.05 * torch.randn((N, DIM), generator=g, device="cuda")).to(torch.float16)
    at = torch.randperm(N // 50, generator=g, device="cuda")[:400]
    rows[at] = _planted(u, g, 400, 1.0, 2.0)
    return rows, _near(u, g, 0.05)


def outlier_blocks():
    """One row of 100 x the background's magnitude in every 256-row block (pointing away from the queries, so it never wins): the block
    scale is the outlier's, the background quantises to zeros and ones, eps is about the norm of a background row and the error of an
    estimate is large.  The true top-k rows (scores 6 .. 10, a few quantisation steps per element) are planted inside such blocks, 300 all
    over the index and 160 in the dense segment -- so that tau - eps is above the background from the first int8 segment on; without those
    the int8 filter passes every row and the query overflows, which the fp16 filter does not.  A winner whose estimate falls short of tau
    by more than margin * eps waits in pending until the end."""
    g = _gen(3)
    u = _unit(g)
    rows = (0.05 * torch.randn((N, DIM), generator=g, device="cuda")).to(torch.float16)
    at = torch.arange(17, N, 256, device="cuda")
    x = 5.0 * torch.randn((at.numel(), DIM), generator=g, device="cuda", dtype=torch.float64)
    x = x - (x @ u)[:, None] * u[None, :] - 40.0 * u[None, :]
    rows[at] = x.to(torch.float16)
    win = torch.cat([torch.randperm(N, generator=g, device="cuda")[:300], torch.randperm(8192, generator=g, device="cuda")[:160]])
    win = win[(win % 256) != 17]
    rows[win] = _planted(u, g, win.numel(), 6.0, 10.0)
    return rows, _near(u, g, 0.02)


def crowded_band(kp=64):
    """kp clear winners inside the first 8,192 rows (scores 1.6, .., 2.0: 64 of them for k <= 56, 128 for k = 120, so that the kp-th best is
    the weakest winner either way and every query stays provable) and, behind them, 18,000 rows spread over the rest of the index whose
    scores lie in a band of width 0.023 just below the weakest winner's 1.6.  With q ~ u (|u_i| <~ 0.19) and row norms <= 1.6,
    eps = a_q N_b + b_q D_b ~ 0.007 * 1.6 + 0.011 = 0.022 (quantisation steps t = 0.19 / 127, s = 1.6 * 0.19 / 127, error step * sqrt(256 / 12)):
    the fp16 filter passes none of the band, the int8 filter most of it, ~12,500 rows per query with an estimate in
    [tau - eps, tau - eps / 4): the pending list (8,192) fills up -- the re-score-in-place path -- and the last segment's sub-lists (1,024
    entries each, ~1,130 survivors per XCD) spill into the main list.  test_crowded_band_fills_the_pending_list counts both on the numpy
    model of the filter."""
    g = _gen(4)
    u = _unit(g)
    rows = (0.02 * torch.randn((N, DIM), generator=g, device="cuda")).to(torch.float16)
    at = torch.randperm(8192, generator=g, device="cuda")[:kp]
    c = torch.linspace(1.6, 2.0, kp, device="cuda", dtype=torch.float64)[:, None]
    rows[at] = (c * u[None, :] + 0.0005 * torch.randn((kp, DIM), generator=g, device="cuda", dtype=torch.float64)).to(torch.float16)
    band = 8192 + torch.randperm(N - 8192, generator=g, device="cuda")[:18_000]
    c = 1.597 - 0.023 * torch.rand((18_000, 1), generator=g, device="cuda", dtype=torch.float64)
    rows[band] = (c * u[None, :] + 0.0005 * torch.randn((18_000, DIM), generator=g, device="cuda", dtype=torch.float64)).to(torch.float16)
    return rows, _near(u, g, 0.0005)


def degenerate_constants():
    """Zero queries (t_q = 0: estimate and bound are 0), all-zero 256-row blocks (s_b = 0: every row of the block survives with U = 0) inside
    int8 segments, queries equal to a row (their own row is the clear winner), a tiny and a large query.  Every score of a zero query is
    0 = tau, every row passes either filter and the query overflows on BOTH paths whatever the size: the one exception to "no overflow",
    made for the queries of ZERO_QUERIES only."""
    g = _gen(5)
    rows = torch.randn((N, DIM), generator=g, device="cuda").to(torch.float16)
    rows[256 * 300:256 * 301] = 0
    rows[256 * 700:256 * 702] = 0
    q = torch.randn((NQ_MAX, DIM), generator=g, device="cuda").to(torch.float16)
    q[3] = 0
    q[4] = rows[200_000]
    q[5] = rows[N - 5]
    q[6] = (q[6].double() * 2.0 ** -12).to(torch.float16)
    q[7] = (q[7].double() * 100.0).to(torch.float16)
    q[129] = 0                                                           # (the last query of the 130-query case)
    return rows, q


def duplicates():
    """A quarter of the rows are exact copies of other rows, as in the existing suite: ties that only the row order breaks, across the kp
    boundary and between a row re-scored at once and its copy re-scored at the end."""
    g = _gen(6)
    rows = torch.randn((N, DIM), generator=g, device="cuda").to(torch.float16)
    src = torch.randint(0, N, (N // 4,), generator=g, device="cuda")
    dst = torch.randint(0, N, (N // 4,), generator=g, device="cuda")
    rows[dst] = rows[src]
    return rows, torch.randn((NQ_MAX, DIM), generator=g, device="cuda").to(torch.float16)


ZERO_QUERIES = (3, 129)                                                  # of degenerate_constants
FAMILIES = {f.__name__: f for f in (late_winners, early_winners, outlier_blocks, crowded_band, degenerate_constants, duplicates)}
_cache = {}


def _family(name, kp=64):
    """(shard with shadow, fp16-only shard, queries, rows): built once per family (crowded_band: per kp), never modified"""
    key = (name, kp if name == "crowded_band" else 0)
    if key not in _cache:
        _cache.clear()                                                   # (one family's shards at a time)
        rows, q = FAMILIES[name](kp) if name == "crowded_band" else FAMILIES[name]()
        assert torch.isfinite(rows.float()).all()
        ids = torch.randperm(N, generator=_gen(99), device="cuda").to(torch.int32) + 1
        sa, sb = _pair(rows, ids, BASE, min_rows=MIN_ROWS)
        assert sa._shadow is not None
        _cache[key] = (sa, sb, q, rows)
    return _cache[key]


@pytest.mark.parametrize("k", [1, 50, 120])
@pytest.mark.parametrize("nq", [130, 512])
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_deferred_rescore_changes_nothing(family, nq, k):
    sa, sb, q_all, _ = _family(family, 64 if k <= 56 else 128)
    q = q_all[:nq].contiguous()
    n0 = _launches()
    a = sa.search(q, k, exact_fallback=False)
    assert _launches() - n0 >= 2, "the int8 segments did not run"
    b = sb.search(q, k, exact_fallback=False)
    over = set(torch.nonzero(b[3] & 2).flatten().tolist())
    allowed = set(j for j in ZERO_QUERIES if j < nq) if family == "degenerate_constants" else set()
    assert over <= allowed, "the fp16-only shard overflowed (queries %s): the case tests the fallback, not the deferred pass" % sorted(over - allowed)
    _assert_same(a, b, "(search)")
    _assert_same(sa.search_f32(q, k, exact_fallback=False), sb.search_f32(q, k, exact_fallback=False), "(search_f32)")
    for f32 in (False, True):
        ra, fa = sa.search_records(q, k, f32=f32, exact_fallback=False)
        rb, fb = sb.search_records(q, k, f32=f32, exact_fallback=False)
        keep = (fa & 2) == 0
        assert torch.equal(fa & 2, fb & 2) and torch.equal(fa[keep], fb[keep]) and torch.equal(ra[keep], rb[keep]), "records differ (f32=%s)" % f32
    # five sampled queries against the all-exact integer path
    d, i, r, f = a
    sel = torch.tensor(sorted(set([0, 4, nq // 2, nq - 2, nq - 1])), dtype=torch.int32, device="cuda")
    d2, i2, r2, f2 = d.clone(), i.clone(), r.clone(), f.clone()
    d2[sel.long()] = 0; i2[sel.long()] = -7; r2[sel.long()] = -7
    sa.search_exact(q, sel, k, d2, i2, r2, f2)
    ok = (f & 2) == 0                                                    # (a zero query's provisional payload is whatever its overflowed list kept)
    _assert_same((d[ok], i[ok], r[ok]), (d2[ok], i2[ok], r2[ok]), "(vs all-exact)")


@pytest.mark.parametrize("kp", [64, 128])
def test_crowded_band_fills_the_pending_list(kp):
    """What crowded_band is for, counted on the numpy restatement of the filter (tools/mips_i8_filter_study.py) for the rows the GPU cases
    search: walking the segments with tau = the kp-th best exact score so far, more than 8,192 survivors per query have an estimate in
    [tau - eps, tau - eps / 4) -- deferred by any margin up to eps / 4 -- in the two int8 segments of the 130-query cases already, and in the
    last segment some XCD's eighth of the rows holds more than 1,024 survivors: that sub-list spills into the main list."""
    import importlib.util
    import os
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mips_i8_filter_study", os.path.join(root, "tools", "mips_i8_filter_study.py"))
    st = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(st)
    _, _, q_all, rows_gpu = _family("crowded_band", kp)
    rows, q = rows_gpu.cpu().numpy(), q_all[[0, 129, 511]].cpu().numpy()
    e8, blk = st.quantise_blocks(rows)
    q8, qc = st.quantise_queries(q)
    blk_of = np.arange(N) // st.BLOCK
    est = qc[:, 0:1].astype(np.float64) * blk[blk_of, 0].astype(np.float64)[None, :] * st.int_scores(e8, q8)
    eps = st.epsilon(qc, blk).astype(np.float64)[:, blk_of]
    S = q.astype(np.float64) @ rows.astype(np.float64).T
    for j in range(len(q)):
        best = np.sort(S[j, :65536])[-kp:]
        deferred = 0
        for lo, hi in ((65536, 131072), (131072, N)):
            tau = best[0]
            passed = est[j, lo:hi] >= tau - eps[j, lo:hi]
            deferred += int((passed & (est[j, lo:hi] + 0.25 * eps[j, lo:hi] < tau)).sum())
            best = np.sort(np.concatenate([best, S[j, lo:hi][passed]]))[-kp:]
        assert deferred > 8192, "query %d: only %d deferred survivors" % (j, deferred)
        assert max(int(c.sum()) for c in np.array_split(passed, 8)) > 1024
