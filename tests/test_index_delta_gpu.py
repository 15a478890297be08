"""GPU: incremental index snapshots -- emdr2_mips_row_keys against its numpy restatement bit for bit, emdr2_mips_changed_rows against
`np.flatnonzero(host keys now != base keys)` over planted sets of changes and over the real row writers, and base + delta through
`save_flat_file(track_deltas=True)` / `save_delta` / `load_flat_snapshot(delta=True)`: digests, stamps, search results, the audit, and the
paced writer with updates on both sides of its cursor."""
import os

import numpy as np
import pytest
import torch

from tests.test_index_generations_cpu import apply_list, apply_range

pytestmark = pytest.mark.gpu
M64 = 2 ** 64 - 1
BASE = 1001                                  # the shards' row_base: the rows reported are GLOBAL rows


def _dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _shard(n, dim, stamped, seed=0):
    """a filled shard numbered from BASE, with random stamps -> (shard, host rows, host stamps or None)"""
    from emdr2_amd.data.emdr2_index import HipIndexShard
    rng = np.random.default_rng(seed + n)
    rows = rng.standard_normal((n, dim)).astype(np.float16)
    sh = HipIndexShard(dim, n, BASE, shadow_min_rows=1, generations=stamped)
    sh.append_rows(rows)
    stamps = None
    if stamped:
        stamps = rng.integers(0, 2 ** 31, size=n, dtype=np.int64).astype(np.uint32)
        stamps[0], stamps[-1] = 0, 2 ** 31 - 1
        sh.set_stamps(0, stamps)
    return sh, rows, stamps


# ---- the keys ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stamped", [False, True])
@pytest.mark.parametrize("n,dim", [(1, 64), (127, 64), (128, 96), (129, 64), (513, 96), (8492, 768)])
def test_device_row_keys_equal_the_numpy_restatement(n, dim, stamped):
    from emdr2_amd.data.emdr2_index import row_keys
    sh, rows, stamps = _shard(n, dim, stamped)
    want = row_keys(rows, stamps, BASE)
    keys = sh.row_keys()
    assert keys.dtype == torch.int64 and keys.shape == (n,) and np.array_equal(_u64(keys), want)
    # the sum and xor of the keys are the shard's digests
    s, x = sh.digest()
    if stamped:
        gs, gx = sh.digest_stamps()
        with np.errstate(over="ignore"):
            h = want - row_keys(rows, None, BASE)
        assert (int(h.sum(dtype=np.uint64)), int(np.bitwise_xor.reduce(h))) == (gs, gx)
    else:
        assert (int(want.sum(dtype=np.uint64)), int(np.bitwise_xor.reduce(want))) == (s, x)


@pytest.mark.parametrize("stamped", [False, True])
def test_a_sub_range_writes_only_its_own_slots(stamped):
    from emdr2_amd.data.emdr2_index import row_keys
    n = 513
    sh, rows, stamps = _shard(n, 96, stamped)
    sentinel = 0x5555555555555555
    out = torch.full((n,), sentinel, dtype=torch.int64, device="cuda")
    got = sh.row_keys(5, 130, out=out)                                                     # two stripes, both partly covered
    assert got.data_ptr() == out.data_ptr()
    want = np.full(n, sentinel, np.uint64)
    want[5:135] = row_keys(rows[5:135], None if stamps is None else stamps[5:135], BASE + 5)
    assert np.array_equal(_u64(out), want)
    sh.row_keys(n, 0, out=out); sh.row_keys(0, 0, out=out)                                 # empty ranges: nothing is written
    assert np.array_equal(_u64(out), want)
    for call in (lambda: sh.row_keys(5, n), lambda: sh.row_keys(-1, 3), lambda: sh.row_keys(out=out[:-1]),
                 lambda: sh.row_keys(out=torch.zeros(n, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            call()


# ---- the changed rows: planted sets --------------------------------------------------------------------------------------------------------
def _check(sh, base_dev, base_host, rows, stamps):
    """changed_rows at cap 0, n_changed - 1, n_changed and n_rows, twice each, against the host keys of (rows, stamps) -> the changed
    LOCAL rows"""
    from emdr2_amd.data.emdr2_index import row_keys
    n = sh.n_rows
    want = np.flatnonzero(row_keys(rows, stamps, BASE) != base_host).astype(np.int64)
    kept = base_dev.clone()
    digests = list(sh.digest()) + (list(sh.digest_stamps()) if stamps is not None else [0, 0])
    for cap in sorted({0, max(want.size - 1, 0), want.size, n}):
        for _ in range(2):
            got, info = sh.changed_rows(base_dev, cap)
            got, info = got.cpu().numpy(), [w & M64 for w in info.tolist()]
            stored = min(want.size, cap)
            assert got.shape == (cap,) and np.array_equal(got[:stored], want[:stored] + BASE) and bool((got[stored:] == -1).all()), (cap, want.size)
            assert info[:2] == [want.size, stored] and info[6] == (int(want[0]) + BASE if want.size else M64) and info[7] == 0
            assert info[2:6] == digests
    assert torch.equal(base_dev, kept)                                                     # the base keys are read, never written
    return want


# 8,492 rows: 67 stripes, one per workgroup of the write launch, the last one partly filled.  270,001 rows: 2,110 stripes over
# MIPS_DELTA_MAX_SLABS = 512 slabs (csrc/mips_kernels.h) -> 5 stripes per workgroup, 422 workgroups; a workgroup ranks 4 stripes per
# round, so its slab takes two rounds, the second one partly filled.
@pytest.mark.parametrize("n,dim", [(8492, 96), (270001, 64)])
def test_changed_rows_on_planted_sets(n, dim):
    from emdr2_amd.data.emdr2_index import row_keys
    sh, rows0, stamps0 = _shard(n, dim, True)
    base_dev = sh.row_keys()
    base_host = row_keys(rows0, stamps0, BASE)
    assert np.array_equal(_u64(base_dev), base_host)
    rng = np.random.default_rng(7 * n + 1)                                                 # (not the seed of the shard's own rows)
    stripes = (n + 127) // 128

    def fresh(k):
        return rng.standard_normal((k, dim)).astype(np.float16)

    def plant(ids, new_rows=None, new_stamps=None, expect=None):
        """write, check, write back, check that nothing reports"""
        ids = np.asarray(ids, dtype=np.int64)
        rows, stamps = rows0.copy(), stamps0.copy()
        if new_rows is not None:
            rows[ids] = new_rows
            sh.update_rows_at(_dev(ids, np.int64), _dev(new_rows, np.float16), generation=0)
        stamps[ids] = new_stamps if new_stamps is not None else stamps0[ids]
        sh.set_stamps_at(_dev(ids, np.int64), stamps[ids])
        got = _check(sh, base_dev, base_host, rows, stamps)
        assert np.array_equal(got, np.sort(ids) if expect is None else expect)
        sh.update_rows_at(_dev(ids, np.int64), _dev(rows0[ids], np.float16), generation=0)
        sh.set_stamps_at(_dev(ids, np.int64), stamps0[ids])
        assert _check(sh, base_dev, base_host, rows0, stamps0).size == 0                  # changed and changed back: not reported

    assert _check(sh, base_dev, base_host, rows0, stamps0).size == 0                      # none
    plant([0], fresh(1))                                                                   # row 0 only
    plant([n - 1], fresh(1))                                                               # the last row only
    plant(np.arange(n), fresh(n))                                                          # every row
    one = np.arange(stripes) * 128 + rng.integers(0, 128, size=stripes)                    # exactly one row per stripe
    one[-1] = min(one[-1], n - 1)
    plant(one, fresh(stripes))
    s = (stripes // 2) * 128
    plant([s + 17, s + 17 + 64], fresh(2))                                                 # rows r and r + 64 of one stripe: one thread's two rows
    flipped = rows0[[777]].copy()
    flipped.view(np.uint16)[0, -1] ^= 0x0001                                               # one bit in the last element of a row
    plant([777], flipped)
    plant([5, n - 2], None, np.array([stamps0[5] ^ 1, (stamps0[n - 2] + 1) & 0x7fffffff], np.uint32))   # a stamp-only change
    a, b = 300, n - 300
    plant([a, b], rows0[[b, a]], stamps0[[b, a]])                                          # two rows' contents swapped: both report
    # the same bits re-written under the same stamps are no change
    plant([9, 10], rows0[[9, 10]], expect=np.empty(0, np.int64))


def test_changed_rows_without_stamps_and_its_refusals():
    from emdr2_amd.data.emdr2_index import row_keys
    n, dim = 1003, 64
    sh, rows0, _ = _shard(n, dim, False)
    base_dev, base_host = sh.row_keys(), row_keys(rows0, None, BASE)
    assert _check(sh, base_dev, base_host, rows0, None).size == 0
    rows = rows0.copy()
    ids = np.array([0, 127, 128, 640, n - 1], np.int64)
    rows[ids] = np.random.default_rng(1).standard_normal((ids.size, dim)).astype(np.float16)
    sh.update_rows_at(_dev(ids, np.int64), _dev(rows[ids], np.float16))
    assert np.array_equal(_check(sh, base_dev, base_host, rows, None), ids)
    got, info = sh.changed_rows(base_dev, 10 * n)                                          # cap is clamped to the shard's rows
    assert got.shape == (n,) and info.tolist()[:2] == [ids.size, ids.size]
    for call in (lambda: sh.changed_rows(base_dev, -1), lambda: sh.changed_rows(base_dev[:-1], 1), lambda: sh.changed_rows(base_dev.int(), 1),
                 lambda: sh.changed_rows(_u64(base_dev), 1)):
        with pytest.raises(ValueError):
            call()
    sh.begin_refresh()
    with pytest.raises(ValueError, match="refresh"):
        sh.changed_rows(base_dev, 1)
    from emdr2_amd.data.emdr2_index import HipIndexShard
    filling = HipIndexShard(dim, n, 0)
    filling.append_rows(rows0[:100])
    with pytest.raises(ValueError, match="populated"):
        filling.changed_rows(base_dev, 1)
    with pytest.raises(ValueError):
        sh.set_stamps_at(_dev([0], np.int64), np.zeros(1, np.uint32))                      # no stamps on this shard


# ---- the changed rows: the real writers ----------------------------------------------------------------------------------------------------
def test_changed_rows_after_the_real_writers():
    """8,492 x 768 with a sealed shadow: a stamped range update, a stamped scattered update, and a newest-wins range update across rows
    the scattered one has just stamped higher -- those are kept, image and stamp, and are not reported on its account."""
    from emdr2_amd.data.emdr2_index import row_keys
    n, dim = 8492, 768
    sh, rows0, _ = _shard(n, dim, True)
    stamps0 = np.full(n, 3, np.uint32)
    sh.set_stamps(0, stamps0)
    assert sh._shadow is not None
    base_dev, base_host = sh.row_keys(), row_keys(rows0, stamps0, BASE)
    rng = np.random.default_rng(4)
    live, live_stamps = rows0.copy(), stamps0.astype(np.int64)
    new = rng.standard_normal((300, dim)).astype(np.float16)
    sh.update_rows(1000, _dev(new, np.float16), generation=10)
    apply_range(live, live_stamps, 1000, new, 10, False)
    ids = rng.choice(np.arange(4000, 4400), size=120, replace=False).astype(np.int64)
    new = rng.standard_normal((120, dim)).astype(np.float16)
    sh.update_rows_at(_dev(ids - 0, np.int64), _dev(new, np.float16), generation=20)
    apply_list(live, live_stamps, ids, new, 20, False)
    new = rng.standard_normal((600, dim)).astype(np.float16)
    sh.update_rows(3900, _dev(new, np.float16), generation=15, newest_wins=True)
    kept = apply_range(live, live_stamps, 3900, new, 15, True)
    assert kept == 120 == sh.kept_newer()
    got = _check(sh, base_dev, base_host, live, live_stamps.astype(np.uint32))
    want = np.unique(np.concatenate([np.arange(1000, 1300), np.arange(3900, 4500)]))
    assert np.array_equal(got, want)                                                       # (the kept rows report: the scattered update changed them)
    # a newest-wins update that keeps EVERY row it names changes nothing: measured against keys taken after the writes above
    mid_dev, mid_host = sh.row_keys(), row_keys(live, live_stamps.astype(np.uint32), BASE)
    new = rng.standard_normal((ids.size, dim)).astype(np.float16)
    sh.update_rows_at(_dev(ids, np.int64), _dev(new, np.float16), generation=19, newest_wins=True)
    assert sh.kept_newer() == ids.size
    assert _check(sh, mid_dev, mid_host, live, live_stamps.astype(np.uint32)).size == 0
    # ... and one that keeps some: only the rows it wrote report
    span = np.arange(4350, 4450)
    new = rng.standard_normal((span.size, dim)).astype(np.float16)
    sh.update_rows(4350, _dev(new, np.float16), generation=19, newest_wins=True)
    kept = apply_range(live, live_stamps, 4350, new, 19, True)
    assert 0 < kept < span.size and sh.kept_newer() == kept
    got = _check(sh, mid_dev, mid_host, live, live_stamps.astype(np.uint32))
    assert np.array_equal(got, np.setdiff1d(span, ids)) and got.size == span.size - kept
    audit = sh.audit()
    assert audit["sound"] and audit["canonical"] and audit["shadow_in_use"]


# ---- base + delta at the index level ---------------------------------------------------------------------------------------------------------
def _index(dim, generations):
    from emdr2_amd.data import emdr2_index as ei

    class Index(ei.DistributedBruteForceIndex):
        def _make_shard(self, dim, n, base):
            return ei.HipIndexShard(dim, n, base, shadow_min_rows=1, generations=self.generations)
    return Index(embed_size=dim, embed_data=None, use_gpu=True, generations=generations)


def _change(index, rng, n, dim, generation, fraction=0.03):
    """about `fraction` of the rows through a range update and a scattered one (stamped on an index with stamps)"""
    k = max(int(n * fraction / 2), 2)
    lo = int(rng.integers(0, n - k))
    g = (lambda v: v) if index.generations else (lambda v: None)
    index.update_rows(lo, _dev(rng.standard_normal((k, dim)), np.float16), generation=g(generation))
    ids = rng.choice(n, size=k, replace=False).astype(np.int64)
    ids[0], ids[1] = 0, n - 1
    index.update_rows_at(_dev(ids, np.int64), _dev(rng.standard_normal((k, dim)), np.float16), generation=g(generation + 1))


def _same_index(a, b, queries):
    from emdr2_amd.data.index_snapshot import index_digest, index_stamp_digest
    assert index_digest(a) == index_digest(b)
    if a.generations:
        assert index_stamp_digest(a) == index_stamp_digest(b) and torch.equal(a.shard.generation, b.shard.generation)
    for k in (4, 50):
        da, ia = a.search_mips_index(queries, k)
        db, ib = b.search_mips_index(queries, k)
        assert torch.equal(da, db) and torch.equal(ia, ib)


@pytest.mark.parametrize("generations", [False, True])
@pytest.mark.parametrize("n,dim", [(1003, 64), (8492, 768)])
def test_base_plus_delta_is_the_live_index(tmp_path, n, dim, generations):
    from emdr2_amd.data import index_snapshot as snap
    rng = np.random.default_rng(n + generations)
    rows = rng.standard_normal((n, dim)).astype(np.float16)
    ids = (rng.permutation(n) + 1).astype(np.int32)
    queries = _dev(rng.standard_normal((9, dim)), np.float16)
    live = _index(dim, generations)
    live.add_arrays(ids, rows)
    path = str(tmp_path / "snap.flat")
    live.save_flat_file(path, meta={"iteration": 5}, track_deltas=True)
    base_meta = snap.read_snapshot_meta(path)
    assert live.delta_base["base"] == snap.base_of(base_meta)
    _change(live, rng, n, dim, 10)
    said = []
    meta = live.save_delta(path, {"iteration": 12}, log=said.append)
    assert 0.02 * n < meta["m"] <= 0.03 * n + 2 and meta["base"] == snap.base_of(base_meta) and meta["iteration"] == 12
    assert len(said) == 1 and "%d of %d rows" % (meta["m"], n) in said[0] and meta["result"]["digest_sum"] in said[0]
    names = ["snap.flat", "snap.flat.delta", "snap.flat.delta.meta"] + (["snap.flat.gen"] if generations else []) + ["snap.flat.meta"]
    assert sorted(os.listdir(str(tmp_path))) == names
    assert snap.DeltaFile(snap.delta_path(path)).stamped == generations

    fresh = _index(dim, generations)
    out = fresh.load_flat_snapshot(path, audit=True, delta=True)
    assert fresh.delta_applied == meta and "delta_skipped" not in out
    _same_index(fresh, live, queries)
    audit = fresh.audit()
    assert audit["sound"] and audit["canonical"] and audit["shadow_in_use"] == (n == 8492)
    alone = _index(dim, generations)                                                       # the base alone is the index of iteration 5
    alone.load_flat_snapshot(path)
    assert snap.index_digest(alone) == (int(base_meta["digest_sum"], 16), int(base_meta["digest_xor"], 16)) != snap.index_digest(live)

    # a second delta after more changes overwrites the first and loads to the new live state
    _change(live, rng, n, dim, 20)
    meta2 = live.save_delta(path, {"iteration": 14})
    assert meta2["m"] > meta["m"] and meta2["base"] == meta["base"] and sorted(os.listdir(str(tmp_path))) == names
    again = _index(dim, generations)
    again.load_flat_snapshot(path, audit=True, delta=True, max_iteration=14)
    assert again.delta_applied == meta2
    _same_index(again, live, queries)
    # too new for a checkpoint of iteration 13: skipped, the base alone
    early = _index(dim, generations)
    out = early.load_flat_snapshot(path, delta=True, max_iteration=13)
    assert early.delta_applied is None and "iteration 14" in out["delta_skipped"] and snap.index_digest(early) == snap.index_digest(alone)

    # the resumed index's own next delta is relative to the SAME base, and correct
    for index in (again, live):
        _change(index, np.random.default_rng(99), n, dim, 30)
    meta3 = again.save_delta(path, {"iteration": 16})
    assert meta3["base"] == meta["base"] and meta3["m"] > meta2["m"]
    last = _index(dim, generations)
    last.load_flat_snapshot(path, audit=True, delta=True)
    assert last.delta_applied == meta3
    _same_index(last, live, queries)
    # more than max_fraction changed: nothing is written and the stale delta is gone
    assert live.save_delta(path, {"iteration": 17}, max_fraction=0.01, log=said.append) is None
    assert "skipped" in said[-1] and not os.path.exists(snap.delta_path(path)) and not os.path.exists(snap.delta_meta_path(path))


# ---- point in time: the paced writer ---------------------------------------------------------------------------------------------------------
def _marked(rng, k, dim, g):
    """k fresh rows that carry fp16(g) in element 0"""
    new = rng.standard_normal((k, dim)).astype(np.float16)
    new[:, 0] = np.float16(g)
    return new


def test_a_paced_tracked_snapshot_plus_its_delta_is_the_live_index(tmp_path):
    """5,000 x 64, 1,000 rows per pump, stamped updates between the pumps on both sides of the cursor (the pattern of
    tests/test_index_snapshot_stamps_gpu.py; every row written at generation g carries fp16(g) in element 0).  The base on disk is a mix
    of stream points; its keys are those of exactly the bits in the file, so the delta holds exactly the rows that moved on."""
    from emdr2_amd.data import index_snapshot as snap
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile, row_keys
    n, dim = 5000, 64
    rng = np.random.default_rng(9)
    first = _marked(rng, n, dim, 1)
    index = _index(dim, True)
    index._load_generation = 1
    index.add_arrays(np.arange(1, n + 1, dtype=np.int32), first)
    sh = index.shard
    live, live_stamps = first.copy(), np.full(n, 1, dtype=np.int64)
    writer = snap.IndexSnapshotWriter(index, chunk_rows=1000, track_deltas=True)
    path = str(tmp_path / "snap.flat")
    writer.begin(path, {"iteration": 40, "mode": "rolling"})
    g = 10
    while True:
        c = writer._cursor
        g += 2
        lo, hi = max(c - 150, 0), min(c + 150, n)                                          # a stamped range update across the cursor
        new = _marked(rng, hi - lo, dim, g)
        sh.update_rows(lo, _dev(new, np.float16), generation=g)
        apply_range(live, live_stamps, lo, new, g, False)
        pool = np.arange(max(c - 600, 0), min(c + 600, n))                                 # a scattered one, ids on both sides
        ids = rng.choice(pool, size=80, replace=False).astype(np.int64)
        new = _marked(rng, 80, dim, g + 1)
        sh.update_rows_at(_dev(ids, np.int64), _dev(new, np.float16), generation=g + 1)
        apply_list(live, live_stamps, ids, new, g + 1, False)
        assert writer._error is None and index.delta_base is None
        moved = writer._cursor
        if writer.pump():
            break
        if writer._cursor == moved:                                                        # both buffers busy: pump() did nothing and did not block
            torch.cuda.synchronize()
    writer.finish()
    flat, side = FlatEmbeddingFile(path), snap.StampFile(snap.stamps_path(path))
    file_rows, file_stamps = np.array(flat.rows), np.array(side.stamps)
    assert np.array_equal(_u64(index.delta_base["keys"]), row_keys(file_rows, file_stamps, 0))         # the keys of the bits in the file
    stale = np.flatnonzero((file_stamps.astype(np.int64) != live_stamps) | (file_rows.view(np.uint16) != live.view(np.uint16)).any(axis=1))
    assert stale.size > 300                                                                # rows behind the cursor moved on after their export
    meta = index.save_delta(path, {"iteration": 41})
    delta = snap.DeltaFile(snap.delta_path(path))
    assert np.array_equal(delta.rows, stale) and meta["m"] == stale.size
    fresh = _index(dim, True)
    fresh.load_flat_snapshot(path, audit=True, delta=True)
    assert np.array_equal(fresh.shard.export_rows(0, n).cpu().numpy().view(np.uint16), live.view(np.uint16))     # row for row
    assert np.array_equal(fresh.shard.generation.cpu().numpy()[:n].astype(np.int64), live_stamps)             # stamp for stamp
    assert np.array_equal(fresh.shard.export_rows(0, n).cpu().numpy()[:, 0].astype(np.float64), live_stamps.astype(np.float64))
