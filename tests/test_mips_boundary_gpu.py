"""GPU: the fused start and end of a MIPS search (csrc/mips_aux.hip prepare_kernel, finalize_kernel<2>) and the int8 boundaries between them
(csrc/mips_scan8i.hip triage_kernel + select) change no result.  One launch sets a search up (both query images, norms, {t_q, a_q, b_q},
thresholds, counts, flags, zeroed counters); when something is pending, one launch ends it (deferred pass, select, exact re-score, proof).
Every case compares a shard with a shadow image with the same shard fp16-only on search, search_f32 and search_records, fast path alone
(exact_fallback=False, flags included), bit for bit; the fp16-only side must raise no overflow flag.

Dimension 256, a 16,384-row int8 threshold, row_base != 0, permuted ids.  A filter segment runs on the int8 image only if it also has at
least as many work items (256 rows x 256 queries) as the persistent scan has workgroups; `_int8_segments` restates the schedule of
csrc/mips_plan.h for the device's CU count and every case asserts the number of int8 launches it predicts, which is also the number of
PERSISTENT_I8 segments in the library's own plan (emdr2_mips_search_plan).  On a 256-CU device:
  24,575 rows (8,192 + 16,383): the rest behind the dense segment is one row short of the threshold -- no int8 image is packed, nothing pends;
  24,581 rows (8,192 + 16,384 + 5): the int8 query image IS packed, but the one segment (65 row tiles) is too short for the persistent scan;
  73,733 rows (8,192 + 65,536 + 5): exactly one int8 segment at every query count -- its triage is the only one, the finish follows directly;
  290,003 rows: two int8 segments up to 256 queries, three above."""
import numpy as np
import pytest
import torch

from oracle import mips_oracle as mo
from tests.parity import assert_bit_identical
from tests.test_mips_i8_defer_gpu import _gen, _near, _planted, _unit
from tests.test_mips_i8_gpu import MIN_ROWS, _assert_same, _launches, _pair

pytestmark = pytest.mark.gpu

DIM, BASE, NQ_MAX = 256, 77_001, 512
N_NO_INT8, N_SHORT, N_ONE, N_LONG = 8192 + 16383, 8192 + 16384 + 5, 8192 + 65536 + 5, 290_003
LAST_SEGMENT = 131_072                                                   # first row of the last segment at N_LONG


def _int8_segments(n, nq):
    """int8 scan launches of one search of n rows (search_impl's segment schedule: seg0 8,192, growth 8, growth_i8 2)"""
    from emdr2_amd import _native
    if nq <= 128 or n - 8192 < MIN_ROWS:
        return 0
    grid = max(_native.lib().emdr2_device_cu_count() & ~15, 16)
    halves = 1 if nq <= 256 else 2
    done, end, count = 8192, 0, 0
    while done < n:
        end = min(done * (2 if done >= MIN_ROWS else 8), n)
        if n - end < end // 2:
            end = n
        count += end - done >= MIN_ROWS and ((end + 255) // 256 - done // 256) * halves >= grid
        done = end
    return count


def background(n, seed=11):
    g = _gen(seed)
    return torch.randn((n, DIM), generator=g, device="cuda").to(torch.float16), torch.randn((NQ_MAX, DIM), generator=g, device="cuda").to(torch.float16)


def early_winners(n):
    """test_mips_i8_defer_gpu.early_winners at n rows: the winners sit in the dense segment, pending entries all die unread"""
    g = _gen(2)
    u = _unit(g)
    rows = (0.05 * torch.randn((n, DIM), generator=g, device="cuda")).to(torch.float16)
    at = torch.randperm(8192, generator=g, device="cuda")[:400]
    rows[at] = _planted(u, g, 400, 1.0, 2.0)
    return rows, _near(u, g, 0.05)


def crowded_band(n, kp):
    """test_mips_i8_defer_gpu.crowded_band at n rows: kp clear winners in the dense segment and a band of rows (18,000, or 70 % of what lies
    behind the dense segment) just below the weakest winner, which the int8 filter passes and the margin defers: the pending list fills up"""
    g = _gen(4)
    u = _unit(g)
    rows = (0.02 * torch.randn((n, DIM), generator=g, device="cuda")).to(torch.float16)
    at = torch.randperm(8192, generator=g, device="cuda")[:kp]
    c = torch.linspace(1.6, 2.0, kp, device="cuda", dtype=torch.float64)[:, None]
    rows[at] = (c * u[None, :] + 0.0005 * torch.randn((kp, DIM), generator=g, device="cuda", dtype=torch.float64)).to(torch.float16)
    m = min(18_000, (n - 8192) * 7 // 10)
    band = 8192 + torch.randperm(n - 8192, generator=g, device="cuda")[:m]
    c = 1.597 - 0.023 * torch.rand((m, 1), generator=g, device="cuda", dtype=torch.float64)
    rows[band] = (c * u[None, :] + 0.0005 * torch.randn((m, DIM), generator=g, device="cuda", dtype=torch.float64)).to(torch.float16)
    return rows, _near(u, g, 0.0005)


def rising_winners(m):
    """m rows planted in the LAST segment of N_LONG rows only, scores rising with the row number from 1 to 2 above a background below 0.3:
    each beats everything before it, all m pass either filter for every query and all are likely winners of the last triage.  m = 6,000: the
    key set of the select behind it (kp + survivors) stays under SEL_LDS = 8,192; m = 12,000: it does not, an XCD's eighth holds ~1,500 survivors, the
    sub-lists (1,024) spill into the main list and the select reads its keys unstaged.  test_rising_winners_sizes counts both."""
    g = _gen(7)
    u = _unit(g)
    rows = (0.05 * torch.randn((N_LONG, DIM), generator=g, device="cuda")).to(torch.float16)
    at = LAST_SEGMENT + torch.sort(torch.randperm(N_LONG - LAST_SEGMENT, generator=g, device="cuda")[:m]).values
    c = torch.linspace(1.0, 2.0, m, device="cuda", dtype=torch.float64)[:, None]
    rows[at] = (c * u[None, :] + 0.01 * torch.randn((m, DIM), generator=g, device="cuda", dtype=torch.float64)).to(torch.float16)
    return rows, _near(u, g, 0.05)


_cache = {}


def _shards(key, make):
    """(shard with shadow, fp16-only shard, queries, rows, ids): built once per key, one key's shards at a time, never modified"""
    if key not in _cache:
        _cache.clear()
        rows, q = make()
        n = rows.shape[0]
        ids = torch.randperm(n, generator=_gen(99), device="cuda").to(torch.int32) + 1
        sa, sb = _pair(rows, ids, BASE, min_rows=1)                     # (sealed whatever the row count; the searches get the real threshold)
        assert sa._shadow is not None
        sa.shadow_min_rows = MIN_ROWS
        _cache[key] = (sa, sb, q, rows, ids)
    return _cache[key]


def _check(sa, sb, q, k, n):
    """every entry point, fast path alone, against the fp16-only shard; the int8 launches of the first search as the schedule predicts"""
    n0 = _launches()
    a = sa.search(q, k, exact_fallback=False)
    torch.cuda.synchronize()
    ran, want = _launches() - n0, _int8_segments(n, q.shape[0])
    assert ran == want, "int8 scan launches: %d, the schedule says %d" % (ran, want)
    from emdr2_amd import _native
    planned = sum(s[2] == "PERSISTENT_I8" for s in _native.search_plan(n, q.shape[0], DIM, k, MIN_ROWS, _native.lib().emdr2_device_cu_count())[0])
    assert planned == want == ran, "int8 segments: the plan says %d, the restated schedule %d, %d ran" % (planned, want, ran)
    b = sb.search(q, k, exact_fallback=False)
    over = torch.nonzero(b[3] & 2).flatten().tolist()
    assert not over, "the fp16-only shard overflowed (queries %s): the case tests the fallback, not the boundaries" % over
    _assert_same(a, b, "(search)")
    _assert_same(sa.search_f32(q, k, exact_fallback=False), sb.search_f32(q, k, exact_fallback=False), "(search_f32)")
    for f32 in (False, True):
        ra, fa = sa.search_records(q, k, f32=f32, exact_fallback=False)
        rb, fb = sb.search_records(q, k, f32=f32, exact_fallback=False)
        assert torch.equal(fa, fb) and torch.equal(ra, rb), "records differ (f32=%s)" % f32
    return a


@pytest.mark.parametrize("k", [1, 50, 120])
@pytest.mark.parametrize("nq", [129, 257, 512])
@pytest.mark.parametrize("n", [N_NO_INT8, N_SHORT, N_ONE, N_LONG])
def test_row_and_query_counts_that_move_the_boundaries(n, nq, k):
    sa, sb, q_all, _, _ = _shards(("background", n), lambda: background(n))
    _check(sa, sb, q_all[:nq].contiguous(), k, n)


@pytest.mark.parametrize("k", [1, 50, 120])
@pytest.mark.parametrize("nq", [129, 512])
@pytest.mark.parametrize("m", [6_000, 12_000])
def test_many_likely_winners_in_the_last_segment(m, nq, k):
    sa, sb, q_all, _, _ = _shards(("rising", m), lambda: rising_winners(m))
    _check(sa, sb, q_all[:nq].contiguous(), k, N_LONG)


@pytest.mark.parametrize("m", [6_000, 12_000])
def test_rising_winners_sizes(m):
    """What the two sizes are for, counted on the numpy restatement of the filter (tools/mips_i8_filter_study.py) over the last segment, with
    tau = the kp-th best exact score of the rows before it (the tau the segment is scanned with): the survivors are at least the m planted
    rows, with the kp kept entries they stay under SEL_LDS at 6,000 and pass it at 12,000, where an eighth of the segment also holds more
    than SUBCAP of them; either way they fit the 16,384 + 8 x 1,024 slots a query has."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("mips_i8_filter_study", os.path.join(root, "tools", "mips_i8_filter_study.py"))
    st = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(st)
    _, _, q_all, rows_gpu, _ = _shards(("rising", m), lambda: rising_winners(m))
    q = q_all[[0, 128, 511]].cpu().numpy()
    head = (q_all[[0, 128, 511]].double() @ rows_gpu[:LAST_SEGMENT].double().T).cpu().numpy()
    rows = rows_gpu[LAST_SEGMENT:].cpu().numpy()
    e8, blk = st.quantise_blocks(rows)
    q8, qc = st.quantise_queries(q)
    blk_of = np.arange(rows.shape[0]) // st.BLOCK
    est = qc[:, 0:1].astype(np.float64) * blk[blk_of, 0].astype(np.float64)[None, :] * st.int_scores(e8, q8)
    eps = st.epsilon(qc, blk).astype(np.float64)[:, blk_of]
    for kp in (64, 128):
        for j in range(len(q)):
            tau = np.sort(head[j])[-kp]
            passed = est[j] >= tau - eps[j]
            likely = passed & (est[j] + 0.25 * eps[j] >= tau)
            total, worst = int(passed.sum()), max(int(c.sum()) for c in np.array_split(passed, 8))
            assert int(likely.sum()) >= m and total + kp < 16384 + 8 * 1024, (j, total)
            if m == 6_000:
                assert total + kp <= 8192 and worst <= 1024, (j, total, worst)
            else:
                assert total + kp > 8192 and worst > 1024, (j, total, worst)


@pytest.mark.parametrize("k", [50, 120])
@pytest.mark.parametrize("nq", [129, 512])
@pytest.mark.parametrize("n", [N_SHORT, N_ONE])
@pytest.mark.parametrize("family", ["early_winners", "crowded_band"])
def test_pending_empty_and_pending_full_with_one_segment(family, n, nq, k):
    kp = 64 if k <= 56 else 128
    if family == "early_winners":
        sa, sb, q_all, _, _ = _shards((family, n), lambda: early_winners(n))
    else:
        sa, sb, q_all, _, _ = _shards((family, n, kp), lambda: crowded_band(n, kp))
    _check(sa, sb, q_all[:nq].contiguous(), k, n)


@pytest.mark.parametrize("nq", [100, 130, 512])
@pytest.mark.parametrize("n", [N_NO_INT8, N_ONE])
def test_prepare_gives_the_images_and_constants_the_search_is_proven_with(n, nq):
    """prepare_kernel with its int8 part (N_ONE rows, more than 128 queries) and without (N_NO_INT8 rows; 100 queries): the fp16 query
    image, ||q||, thresholds, counts, flags and zeroed counters serve both shards, so the result is also held against the CPU oracle; the
    int8 image and {t_q, a_q, b_q} only the shard with the shadow, whose result must equal the fp16-only shard's bit for bit, proven (flags 0)."""
    sa, sb, q_all, rows, ids = _shards(("background", n), lambda: background(n))
    q = q_all[:nq].contiguous()
    d, i, r, f = _check(sa, sb, q, 50, n)
    assert int(f.abs().sum()) == 0
    od, oi, orow = mo.topk(rows.cpu().numpy(), q.cpu().numpy(), 50, ids=ids.cpu().numpy(), row_base=BASE, return_rows=True)
    assert_bit_identical(d.cpu().numpy(), i.cpu().numpy(), od, oi)
    assert np.array_equal(r.cpu().numpy(), orow)
