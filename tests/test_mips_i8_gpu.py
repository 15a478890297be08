"""GPU: the int8 shadow path of the MIPS search (csrc/mips_scan8i.hip) returns what the fp16 path returns, bit for bit: scores,
ids, rows and flags of a shard with a shadow image against the same shard fp16-only and against the all-exact path / the oracle.  The
"long segment" threshold is lowered through the shard's argument so that the int8 kernel really runs at test sizes -- asserted through the
library's launch counter wherever the shape can take it."""
import hashlib

import numpy as np
import pytest
import torch

from oracle import mips_oracle as mo
from tests.parity import assert_bit_identical
from tests.test_mips_gpu import _search

pytestmark = pytest.mark.gpu

MIN_ROWS = 16384          # filter segments of at least this many rows take the int8 image (production: 512 k)


def _launches():
    from emdr2_amd import _native
    return _native.lib().emdr2_mips_shadow_launches()


def _pair(rows, ids=None, row_base=0, min_rows=MIN_ROWS):
    """(shard with a shadow image, the same shard fp16-only)"""
    from emdr2_amd.data.emdr2_index import HipIndexShard
    out = []
    for shadow in (True, False):
        sh = HipIndexShard(rows.shape[1], rows.shape[0], row_base, shadow=shadow, shadow_min_rows=min_rows)
        sh.append_rows(rows)
        if ids is not None:
            sh.set_ids(ids)
        out.append(sh)
    assert out[1]._shadow is None
    return out


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.float16 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def _assert_same(a, b, what=""):
    """dist, idx, row (and flags when given) bit-identical.  The one exception is the provisional payload of a query whose candidate lists
    OVERFLOWED (flag bit 2, only visible with exact_fallback=False): which survivors an overflowing list lost depends on the order the
    workgroups appended them in, run to run on the fp16 path too, and the contract for such a query is "re-run it exactly".  The flags
    must agree on who overflowed and, for everybody else, bit for bit (the "ambiguous" bit of an overflowed query is derived from that payload)."""
    keep = None
    if len(a) > 3:
        keep = (a[3] & 2) == 0
        assert torch.equal(a[3] & 2, b[3] & 2) and torch.equal(a[3][keep], b[3][keep]), "flags differ %s" % (what,)
    for name, x, y in zip(("dist", "idx", "row"), a, b):
        x, y = _bits(x), _bits(y)
        if keep is not None:
            x, y = x[keep], y[keep]
        assert torch.equal(x, y), "%s differs %s" % (name, what)


def _compare_all_entry_points(sa, sb, q, k, expect_int8):
    """search / search_f32 / search_records (fp16 and fp32 scores), fast path alone (flags included) and with the exact fallback"""
    n0 = _launches()
    for kw in ({"exact_fallback": False}, {}):
        _assert_same(sa.search(q, k, **kw), sb.search(q, k, **kw), "(search %s)" % kw)
        _assert_same(sa.search_f32(q, k, **kw), sb.search_f32(q, k, **kw), "(search_f32 %s)" % kw)
        for f32 in (False, True):
            ra, fa = sa.search_records(q, k, f32=f32, **kw)
            rb, fb = sb.search_records(q, k, f32=f32, **kw)
            keep = (fa & 2) == 0
            assert torch.equal(fa & 2, fb & 2) and torch.equal(fa[keep], fb[keep]) and torch.equal(ra[keep], rb[keep]), "records differ (f32=%s %s)" % (f32, kw)
    torch.cuda.synchronize()
    ran = _launches() - n0
    assert (ran > 0) == expect_int8, "int8 scan launches: %d, expected %s" % (ran, "some" if expect_int8 else "none")


def test_random_shapes_generator_of_the_fp16_suite():
    """The 24 seeded shapes of test_mips_gpu.test_random_shapes_property_vs_oracle through a shard that asks for a shadow image: none of them
    has a segment the persistent scan takes (<= 47 queries, < 6,000 rows), so the dispatch must leave them on the fp16 kernels -- and say so."""
    rng = np.random.default_rng(20260928)
    for case in range(24):
        n = int(rng.integers(1, 6000))
        dim = int(rng.integers(2, 33)) * 32
        nq = int(rng.integers(1, 48))
        k = int(rng.integers(1, 121))
        base = int(rng.integers(0, 1 << 20))
        scale = float(rng.choice([0.01, 0.25, 1.0, 4.0]))
        rows = (rng.standard_normal((n, dim)) * scale).astype(np.float16)
        if n > 10 and case % 3 == 0:
            rows[rng.integers(0, n, size=n // 4)] = rows[rng.integers(0, n, size=n // 4)]
        q = (rng.standard_normal((nq, dim)) * scale).astype(np.float16)
        ids = (rng.permutation(n) + 1).astype(np.int32)
        sa, sb = _pair(rows, ids, base, min_rows=1)
        n0 = _launches()
        d, i, r, f = _search(sa, q, k)
        assert _launches() == n0
        od, oi, orow = mo.topk(rows, q, k, ids=ids, row_base=base, return_rows=True)
        assert (f == 0).all(), case
        assert_bit_identical(d, i, od, oi)
        assert np.array_equal(r, orow), case
        _assert_same(sa.search(torch.from_numpy(q).cuda(), k, exact_fallback=False), sb.search(torch.from_numpy(q).cuda(), k, exact_fallback=False), case)


def test_random_long_shapes_run_the_int8_kernel_and_match():
    """The same generator scaled to shapes the int8 kernel takes (129..512 queries, 140 k .. 400 k rows, dim a multiple of 256): every entry
    point bit-identical to the fp16-only shard, sampled queries bit-identical to the all-exact integer path."""
    rng = np.random.default_rng(20260929)
    for case in range(8):
        n = int(rng.integers(140_000, 400_000))
        dim = int(rng.integers(1, 5)) * 256
        nq = int(rng.integers(129, 513))
        k = int(rng.integers(1, 121))
        base = int(rng.integers(0, 1 << 20))
        scale = float(rng.choice([0.01, 0.25, 1.0, 4.0]))
        g = torch.Generator(device="cuda").manual_seed(1000 + case)
        rows = (torch.randn((n, dim), generator=g, device="cuda") * scale).to(torch.float16)
        if case % 3 == 0:                                               # exact duplicates: ties that only the row order can break
            src = torch.randint(0, n, (n // 4,), generator=g, device="cuda")
            dst = torch.randint(0, n, (n // 4,), generator=g, device="cuda")
            rows[dst] = rows[src]
        q = (torch.randn((nq, dim), generator=g, device="cuda") * scale).to(torch.float16)
        ids = torch.randperm(n, generator=g, device="cuda").to(torch.int32) + 1
        sa, sb = _pair(rows, ids, base)
        assert sa._shadow is not None
        _compare_all_entry_points(sa, sb, q, k, expect_int8=True)
        d, i, r, f = sa.search(q, k)
        sel = torch.tensor(sorted(set([0, 1, nq // 2, nq - 2, nq - 1])), dtype=torch.int32, device="cuda")
        d2, i2, r2, f2 = d.clone(), i.clone(), r.clone(), f.clone()
        d2[sel.long()] = 0; i2[sel.long()] = -7; r2[sel.long()] = -7
        sa.search_exact(q, sel, k, d2, i2, r2, f2)
        _assert_same((d, i, r, f), (d2, i2, r2, f2), "(vs all-exact, case %d)" % case)


@pytest.mark.parametrize("n,dim,nq,k,takes", [
    (1, 64, 1, 1, False), (37, 64, 3, 50, False), (127, 96, 5, 7, False), (129, 768, 2, 50, False), (2048, 768, 17, 50, False),
    (2049, 768, 130, 51, False), (5000, 128, 600, 20, False), (3000, 1024, 9, 120, False), (70000, 256, 64, 101, False),
    (70000, 256, 130, 101, False), (140000, 256, 130, 101, True), (73729, 768, 512, 50, True), (90000, 512, 700, 120, True),
])
def test_edge_shapes(n, dim, nq, k, takes):
    """The edge shapes of test_mips_gpu.test_edge_shapes_vs_oracle -- none of which the int8 kernel can take: too few queries, a dim that is
    no multiple of 256, or no filter segment of 256 work items (256 rows x 256 queries each), which also holds for the tenth shape -- and
    three that it does take, against the fp16-only shard and the oracle.  `takes` is asserted either way."""
    rng = np.random.default_rng(n * 7 + dim + nq)
    rows = rng.standard_normal((n, dim)).astype(np.float16)
    q = rng.standard_normal((nq, dim)).astype(np.float16)
    ids = (rng.permutation(n) + 1).astype(np.int32)
    sa, sb = _pair(rows, ids, 1000, min_rows=1)
    _compare_all_entry_points(sa, sb, torch.from_numpy(q).cuda(), k, expect_int8=takes)
    d, i, r, f = _search(sa, q, k)
    od, oi, orow = mo.topk(rows, q, k, ids=ids, row_base=1000, return_rows=True)
    assert (f == 0).all()
    assert_bit_identical(d, i, od, oi)
    assert np.array_equal(r, orow)


@pytest.mark.parametrize("hot_frac,nq", [(0.01, 300), (0.2, 300), (0.01, 200)])
def test_queue_flush_and_overflow_on_the_int8_kernel(hot_frac, nq):
    """Late rows that beat the running thresholds of every query (test_mips_gpu.test_persistent_filter_scan_queue_flush_and_overflow at a dim
    the int8 kernel takes): mid-kernel queue flushes at 1 %, queue overflow straight to the sub-lists (integer score words on that path
    too), candidate overflow and the exact fallback at 20 %."""
    rng = np.random.default_rng(int(hot_frac * 1000) + nq)
    n, dim, k = 300_000, 256, 50
    u = rng.standard_normal(dim); u /= np.linalg.norm(u)
    q = (u[None, :] + 0.05 * rng.standard_normal((nq, dim))).astype(np.float16)
    rows = (0.05 * rng.standard_normal((n, dim))).astype(np.float16)
    hot = np.nonzero(rng.random(n) < hot_frac)[0]
    hot = hot[hot >= 140_000]
    rows[hot] = (u[None, :] * (1.0 + rng.random((hot.size, 1))) + 0.05 * rng.standard_normal((hot.size, dim))).astype(np.float16)
    sa, sb = _pair(rows)
    _compare_all_entry_points(sa, sb, torch.from_numpy(q).cuda(), k, expect_int8=True)
    d, i, r, f = _search(sa, q, k)
    od, oi, orow = mo.topk(rows, q, k, return_rows=True)
    assert (f == 0).all()
    assert_bit_identical(d, i, od, oi)
    assert np.array_equal(r, orow)


def test_adversarial_row_order_flags_and_falls_back():
    """Rows sorted by increasing score: every row beats the running threshold, the lists overflow.  The int8 path must flag the queries (as the
    fp16 path does) and the fallback must give the oracle's result -- nothing is dropped silently."""
    rng = np.random.default_rng(13)
    n, dim, nq = 160_000, 256, 130
    q = np.zeros((nq, dim), dtype=np.float16); q[:, 0] = 1
    q[:, 1:] = (0.01 * rng.standard_normal((nq, dim - 1))).astype(np.float16)
    rows = (rng.standard_normal((n, dim)) * 0.01).astype(np.float16)
    rows[:, 0] = (np.arange(n) / 64).astype(np.float16)
    sa, sb = _pair(rows)
    n0 = _launches()
    fa = sa.search(torch.from_numpy(q).cuda(), 50, exact_fallback=False)
    assert _launches() > n0
    fb = sb.search(torch.from_numpy(q).cuda(), 50, exact_fallback=False)
    assert bool(((fa[3] & 2) != 0).all()) and bool(((fb[3] & 2) != 0).all())       # every query overflowed, on both paths
    d, i, r, f = _search(sa, q[:4], 50)                              # (the all-exact pass is slow: four queries)
    od, oi = mo.topk(rows, q[:4], 50)
    assert (f == 0).all()
    assert_bit_identical(d, i, od, oi)


def test_a_non_finite_row_keeps_the_shard_on_fp16():
    rng = np.random.default_rng(5)
    n, dim, nq = 100_000, 256, 200
    rows = rng.standard_normal((n, dim)).astype(np.float16)
    rows[77_777, 3] = np.inf
    q = rng.standard_normal((nq, dim)).astype(np.float16)
    sa, sb = _pair(rows)
    assert sa._shadow is None and sa._want_shadow
    _compare_all_entry_points(sa, sb, torch.from_numpy(q).cuda(), 50, expect_int8=False)


def test_refresh_committed_from_rows_written_in_shuffled_order():
    """An in-HBM refresh whose rows arrive in shuffled pieces of odd sizes: the commit seals the new image's shadow; the search after it equals
    a fresh fp16-only shard of the new rows and runs on the int8 image.  A second refresh reuses the buffers the other way round."""
    from emdr2_amd.data.emdr2_index import HipIndexShard
    g = torch.Generator(device="cuda").manual_seed(77)
    n, dim, nq, k = 200_000, 512, 300, 50
    old = torch.randn((n, dim), generator=g, device="cuda").to(torch.float16)
    q = torch.randn((nq, dim), generator=g, device="cuda").to(torch.float16)
    sh = HipIndexShard(dim, n, 0, shadow=True, shadow_min_rows=MIN_ROWS)
    sh.append_rows(old)
    for round_ in range(2):
        new = (torch.randn((n, dim), generator=g, device="cuda") * (0.5 + round_)).to(torch.float16)
        cuts = [0] + sorted(torch.randint(1, n, (23,), generator=g, device="cuda").tolist()) + [n]
        pieces = [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        sh.begin_refresh()
        for j in torch.randperm(len(pieces), generator=g, device="cuda").tolist():
            a, b = pieces[j]
            sh.refresh_rows(a, new[a:b])
        before = sh.search(q, k, exact_fallback=False)                 # the old image (and its shadow) still serves
        sh.commit_refresh()
        assert sh._shadow is not None
        fresh = HipIndexShard(dim, n, 0, shadow=False)
        fresh.append_rows(new)
        n0 = _launches()
        _assert_same(sh.search(q, k, exact_fallback=False), fresh.search(q, k, exact_fallback=False), "(after refresh %d)" % round_)
        assert _launches() > n0
        prev = HipIndexShard(dim, n, 0, shadow=False)
        prev.append_rows(old)
        _assert_same(before, prev.search(q, k, exact_fallback=False), "(before commit %d)" % round_)
        old = new


def test_clustered_corpus_at_4m_rows():
    """The benchmark's clustered corpus (topic-contiguous rows, log-normal norms, queries near the last 2 % of the rows) at 4.2 M rows with
    the production threshold: the int8 segments run, results and flags equal the fp16 path's, sampled queries equal the all-exact path."""
    import bench
    from emdr2_amd.data.emdr2_index import HipIndexShard
    n, k, nq = 4_200_000, 50, 512
    sh = HipIndexShard(768, n, 0)
    for block in bench.synth_rows_clustered(0, n):
        sh.append_rows(block)
    assert sh._shadow is not None
    q = bench.clustered_queries(n, nq)
    n0 = _launches()
    a = sh.search(q, k, exact_fallback=False)
    assert _launches() > n0
    shadow, sh._shadow = sh._shadow, None
    b = sh.search(q, k, exact_fallback=False)
    sh._shadow = shadow
    _assert_same(a, b)
    d, i, r, f = a
    assert int((f != 0).sum()) <= nq // 100
    sel = torch.tensor([j for j in (0, 8, 77, 200, 301, 400, 480, 511) if int(f[j]) == 0], dtype=torch.int32, device="cuda")
    d2, i2, r2, f2 = d.clone(), i.clone(), r.clone(), f.clone()
    d2[sel.long()] = 0; i2[sel.long()] = -7; r2[sel.long()] = -7
    sh.search_exact(q, sel, k, d2, i2, r2, f2)
    _assert_same((d, i, r), (d2, i2, r2), "(vs all-exact)")


def test_shard_counts_1_3_8_give_one_digest():
    from emdr2_amd.data.emdr2_index import HipIndexShard, merge_shard_results, shard_bounds
    g = torch.Generator(device="cuda").manual_seed(31)
    n, dim, nq, k = 480_000, 256, 300, 50
    rows = torch.randn((n, dim), generator=g, device="cuda").to(torch.float16)
    q = torch.randn((nq, dim), generator=g, device="cuda").to(torch.float16)
    ids = torch.randperm(n, generator=g, device="cuda").to(torch.int32) + 1
    digests = set()
    for shadow in (False, True):
        for world in (1, 3, 8):
            parts = []
            n0 = _launches()
            for lo, hi in shard_bounds(n, world):
                s = HipIndexShard(dim, hi - lo, lo, shadow=shadow, shadow_min_rows=MIN_ROWS)
                s.append_rows(rows[lo:hi]); s.set_ids(ids[lo:hi])
                parts.append(s.search(q, k)[:3])
            assert (_launches() - n0 >= world) == shadow
            md, mi, _ = merge_shard_results(torch.stack([p[0] for p in parts]), torch.stack([p[1] for p in parts]), torch.stack([p[2] for p in parts]))
            h = hashlib.sha256()
            h.update(md.cpu().numpy().tobytes()); h.update(mi.cpu().numpy().tobytes())
            digests.add(h.hexdigest())
    assert len(digests) == 1
