"""GPU: index snapshots -- the export and digest kernels against the rows that were packed and the numpy restatement of the digest, the
save / load round trip of a shard with a sealed int8 shadow, and the paced writer under rolling updates."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DIMS = (64, 256, 768)
N_ROWS = (1, 127, 128, 129, 511, 513, 1000)                               # the stripe boundary at 128, the padding boundary at 512
_ROWS = {}


def _rows(dim):
    """One fp16 [1000, dim] matrix per dim, shared (read-only) by every test; a shape takes its first n rows."""
    if dim not in _ROWS:
        m = np.random.default_rng(dim).standard_normal((1000, dim)).astype(np.float16)
        m.setflags(write=False)
        _ROWS[dim] = m
    return _ROWS[dim]


def _build(rows, row_base=0, **kw):
    from emdr2_amd.data.emdr2_index import HipIndexShard
    sh = HipIndexShard(rows.shape[1], rows.shape[0], row_base, **kw)
    sh.append_rows(np.ascontiguousarray(rows))
    return sh


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", N_ROWS)
def test_export_rows_returns_the_packed_rows_bit_for_bit(n, dim):
    m = _rows(dim)[:n]
    sh = _build(m)
    want = torch.from_numpy(m.copy()).cuda()
    assert torch.equal(_bits(sh.export_rows(0, n)), _bits(want))
    for lo, hi in ((120, 140), (127, 129), (n - 1, n), (0, 0), (n, n)):
        if hi > n:
            continue
        got = sh.export_rows(lo, hi - lo)
        assert got.shape == (hi - lo, dim) and got.dtype == torch.float16 and got.is_cuda
        assert torch.equal(_bits(got), _bits(want[lo:hi])), (lo, hi)
    out = torch.full((n + 3, dim), 7.0, dtype=torch.float16, device="cuda")              # a caller's buffer: only its first rows are written
    got = sh.export_rows(0, n, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(_bits(got), _bits(want)) and bool((out[n:] == 7.0).all())
    for lo, cnt in ((-1, 1), (0, n + 1), (n, 1), (1, -1)):
        with pytest.raises(ValueError):
            sh.export_rows(lo, cnt)
        with pytest.raises(ValueError):
            sh.digest(lo, cnt)
    with pytest.raises(ValueError):
        sh.export_rows(0, n, out=torch.empty((n, dim), dtype=torch.float32, device="cuda"))


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("n", N_ROWS)
def test_digest_equals_the_numpy_restatement(n, dim):
    from emdr2_amd.data.emdr2_index import combine_digests, digest_rows
    m = _rows(dim)[:n]
    for base in (0, 70001):
        sh = _build(m, row_base=base)
        whole = digest_rows(m, base)
        assert sh.digest() == whole, (n, dim, base)
        for a in (1, 128, 300):
            if a < n:
                parts = [sh.digest(0, a), sh.digest(a, n - a)]
                assert parts == [digest_rows(m[:a], base), digest_rows(m[a:], base + a)]
                assert combine_digests(parts) == whole
        assert sh.digest(n, 0) == (0, 0)


def test_digest_hashes_bits_not_values():
    from emdr2_amd.data.emdr2_index import digest_rows
    m = _rows(64)[:300].copy()
    u = m.view(np.uint16)
    u[0, :6] = [0x8000, 0x0000, 0x7c00, 0xfc00, 0x7e00, 0x7e01]            # -0.0, +0.0, inf, -inf, two NaN payloads
    u[129, 63] = 0xfe55; u[299, 0] = 0x7dff; u[128, 1] = 0x0001            # more payloads, a subnormal
    sh = _build(m)
    assert sh.digest() == digest_rows(m)
    assert torch.equal(_bits(sh.export_rows(0, 300)), torch.from_numpy(m.view(np.int16)).cuda())
    z = m.copy(); z.view(np.uint16)[0, 0] = 0x0000                         # -0.0 -> +0.0: equal as values, another digest
    assert _build(z).digest() != sh.digest()


def test_a_1000_row_index_in_three_shards_sums_to_the_one_shard_digest():
    from emdr2_amd.data.emdr2_index import combine_digests, shard_bounds
    m = _rows(256)
    one = _build(m).digest()
    parts = [_build(m[lo:hi], row_base=lo).digest() for lo, hi in shard_bounds(1000, 3)]
    assert combine_digests(parts) == one and len(set(parts)) == 3


@pytest.mark.parametrize("dim", (64, 768))
def test_padding_rows_never_enter_the_digest_or_the_export(dim):
    """n_rows = 129: one row into the second stripe, 383 padding rows up to 512.  The same storage first holds a 512-row shard, so the
    padding is anything but zero."""
    from emdr2_amd.data.emdr2_index import digest_rows
    m = _rows(dim)[:512]
    big = _build(m)
    sh = _build(m[:129], row_base=9)
    clean = sh.digest()
    assert sh.tiled.numel() == big.tiled.numel()
    sh.tiled.copy_(big.tiled)                                               # rows 0..128 as before, rows 129..511 now hold data
    assert sh.digest() == clean == digest_rows(m[:129], 9)
    assert sh.digest(100, 29) == digest_rows(m[100:129], 109)
    assert torch.equal(_bits(sh.export_rows(0, 129)), torch.from_numpy(m[:129].view(np.int16).copy()).cuda())


# ---- round trip ----------------------------------------------------------------------------------------------------------------------------
def _index(min_rows=1):
    from emdr2_amd.data import emdr2_index as ei

    class Index(ei.DistributedBruteForceIndex):
        def _make_shard(self, dim, n, base):
            return ei.HipIndexShard(dim, n, base, shadow_min_rows=min_rows)
    return Index


def test_save_and_load_round_trip_of_a_shard_with_a_sealed_shadow(tmp_path):
    """The shadow-carrying shape of tests/test_mips_update_gpu.py (9001 x 256, shadow_min_rows 1): updates in place, a snapshot, a fresh
    index from it.  Everything a search reads is byte-equal, and so are the searches."""
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile
    from emdr2_amd.data.index_snapshot import read_snapshot_meta
    rng = np.random.default_rng(5)
    n, dim = 9001, 256
    m = rng.standard_normal((n, dim)).astype(np.float16)
    m[300] *= 8
    ids = (rng.permutation(n) + 1).astype(np.int32)
    a = _index()(embed_size=dim, embed_data=None, use_gpu=True)
    a.add_arrays(ids, m)
    assert a.shard._shadow is not None
    for lo, cnt in ((0, 1), (250, 12), (300, 1), (8960, 41), (4000, 700)):
        new = rng.standard_normal((cnt, dim)).astype(np.float16)
        a.update_rows(lo, torch.from_numpy(new).cuda())
        m[lo:lo + cnt] = new
    path = str(tmp_path / "snap.flat")
    a.save_flat_file(path, meta={"iteration": 3, "refreshes": 1, "mode": "rolling"})
    flat = FlatEmbeddingFile(path)
    assert np.array_equal(np.asarray(flat.rows).view(np.uint16), m.view(np.uint16)) and np.array_equal(flat.ids, ids)
    meta = read_snapshot_meta(path)
    assert (int(meta["digest_sum"], 16), int(meta["digest_xor"], 16)) == flat.digest() == a.shard.digest()
    assert (meta["mode"], meta["iteration"], meta["world"], meta["n"], meta["dim"]) == ("rolling", 3, 1, n, dim)
    b = _index()(embed_size=dim, embed_data=None, use_gpu=True)
    assert b.load_flat_snapshot(path) == meta
    sa, sb = a.shard, b.shard
    torch.cuda.synchronize()
    assert torch.equal(sa.tiled, sb.tiled) and torch.equal(sa.emax_sq.view(torch.int32), sb.emax_sq.view(torch.int32))
    assert sa._shadow is not None and sb._shadow is not None
    assert torch.equal(sa._shadow[0], sb._shadow[0]) and torch.equal(sa._shadow[1].view(torch.int32), sb._shadow[1].view(torch.int32))
    assert torch.equal(sa.ids, sb.ids)
    for nq in (130, 7):
        q = torch.from_numpy(rng.standard_normal((nq, dim)).astype(np.float16)).cuda()
        ra, rb = sa.search(q, 50), sb.search(q, 50)
        assert torch.equal(_bits(ra[0]), _bits(rb[0])) and torch.equal(ra[1], rb[1]) and torch.equal(ra[2], rb[2])
    # one byte of the rows flipped: the device digest no longer matches the meta
    w = FlatEmbeddingFile(path, mode="r+")
    w.rows.view(np.uint8)[8999, 3] ^= 1
    w.flush(); del w
    with pytest.raises(ValueError, match="digest"):
        _index()(embed_size=dim, embed_data=None, use_gpu=True).load_flat_snapshot(path)


# ---- the paced writer ------------------------------------------------------------------------------------------------------------------
def _paced_index(n=20000, dim=64, seed=3):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, dim)).astype(np.float16)
    ids = (rng.permutation(n) + 1).astype(np.int32)
    index = _index(min_rows=1 << 30)(embed_size=dim, embed_data=None, use_gpu=True)
    index.add_arrays(ids, m)
    return rng, m, ids, index


def _finalize_by_polling(writer):
    it = 0
    while writer.active:                                                    # (the thread only has a few hundred KiB left to write)
        it += 10
        writer.maybe_finalize(it)
        assert it < 10 ** 7


def test_paced_writer_under_rolling_updates_exports_no_torn_row(tmp_path):
    """20,000 rows, 1,500 per pump, `update_rows` between the pumps: ahead of the cursor (the file must hold the NEW row) and behind it
    (the file keeps the OLD row: it was exported before).  Every row of the file is one or the other, whole."""
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile
    from emdr2_amd.data.index_snapshot import IndexSnapshotWriter, read_snapshot_meta
    rng, m, ids, index = _paced_index()
    n, dim = m.shape
    writer = IndexSnapshotWriter(index, chunk_rows=1500)
    path = str(tmp_path / "snap.flat")
    writer.begin(path, {"iteration": 40, "refreshes": 2, "mode": "rolling"})
    assert writer.maybe_finalize(7) is False and writer.maybe_finalize(10) is False
    want, live, ahead_rows, behind_rows, pumps = m.copy(), m.copy(), 0, 0, 0
    while True:
        c = writer._cursor
        for lo, cnt, ahead in ((c + 100, 37, True), (c + 1490, 20, True), (c - 500, 29, False)):      # (c + 1490: across the chunk's end)
            if lo < 0 or lo + cnt > n:
                continue
            new = rng.standard_normal((cnt, dim)).astype(np.float16)
            index.update_rows(lo, torch.from_numpy(new).cuda())
            live[lo:lo + cnt] = new
            if ahead:
                want[lo:lo + cnt] = new; ahead_rows += cnt
            else:
                behind_rows += cnt
        moved = writer._cursor
        assert writer._error is None
        done = writer.pump()
        pumps += writer._cursor != moved
        if done:
            break
        if writer._cursor == moved:                                         # both buffers busy: pump() did nothing and did not block
            torch.cuda.synchronize()
    assert pumps == 14 and ahead_rows > 500 and behind_rows > 300
    _finalize_by_polling(writer)
    flat = FlatEmbeddingFile(path)
    got = np.asarray(flat.rows).view(np.uint16)
    assert np.array_equal(got, want.view(np.uint16)) and np.array_equal(flat.ids, ids)
    old_or_new = (got == m.view(np.uint16)).all(axis=1) | (got == live.view(np.uint16)).all(axis=1)
    assert old_or_new.all() and not np.array_equal(want, live) and not np.array_equal(want, m)
    meta = read_snapshot_meta(path)
    assert (int(meta["digest_sum"], 16), int(meta["digest_xor"], 16)) == flat.digest()      # the device digest of what was exported
    assert meta["mode"] == "rolling" and meta["iteration"] == 40
    assert sorted(os.listdir(str(tmp_path))) == ["snap.flat", "snap.flat.meta"]


def test_paced_writer_in_swap_mode_writes_the_committed_image(tmp_path):
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile
    from emdr2_amd.data.index_snapshot import IndexSnapshotWriter, read_snapshot_meta
    rng, m, ids, index = _paced_index()
    new = rng.standard_normal(m.shape).astype(np.float16)
    index.begin_refresh()
    for lo in range(0, m.shape[0], 7000):
        index.refresh_rows(lo, torch.from_numpy(new[lo:lo + 7000]).cuda())
    index.commit_refresh()
    writer = IndexSnapshotWriter(index, chunk_rows=IndexSnapshotWriter.paced_chunk_rows(m.shape[0], 20))
    path = str(tmp_path / "snap.flat")
    writer.begin(path, {"iteration": 20, "refreshes": 1, "mode": "swap"})
    with pytest.raises(RuntimeError):
        writer.begin(path, {})
    writer.pump(); writer.pump()
    writer.finish()                                                         # the blocking end: the other eight chunks
    assert not writer.active and writer.pump() is True
    flat = FlatEmbeddingFile(path)
    assert np.array_equal(np.asarray(flat.rows).view(np.uint16), new.view(np.uint16))
    meta = read_snapshot_meta(path)
    assert (int(meta["digest_sum"], 16), int(meta["digest_xor"], 16)) == index.shard.digest() == flat.digest()
    # the same path again: overwritten, with a new meta
    index.update_rows(5, torch.from_numpy(m[5:6].copy()).cuda())
    index.save_flat_file(path, {"iteration": 21, "mode": "rolling"})
    assert read_snapshot_meta(path)["iteration"] == 21 and np.array_equal(FlatEmbeddingFile(path).rows[5], m[5])


def test_an_error_of_the_writer_thread_surfaces_from_finish(tmp_path):
    """The background thread cannot write its slice (what an unwritable or vanished directory does to it): `finish()` re-raises, nothing is
    left under the snapshot's name.  A directory that cannot be written at `begin` fails there: rank 0 creates the file in it."""
    from emdr2_amd.data.index_snapshot import IndexSnapshotWriter
    _, m, ids, index = _paced_index(n=3000)
    with pytest.raises(OSError):
        index.save_flat_file(str(tmp_path / "missing" / "snap.flat"))
    writer = IndexSnapshotWriter(index, chunk_rows=500)
    writer.begin(str(tmp_path / "snap.flat"), {"mode": "swap"})

    class _Unwritable(object):
        def __setitem__(self, key, value):
            raise PermissionError(13, "Permission denied")
    writer._file.rows = _Unwritable()
    writer.pump()
    with pytest.raises(PermissionError):
        writer.finish()
    assert not writer.active and os.listdir(str(tmp_path)) == []


# ---- two ranks on one GPU -----------------------------------------------------------------------------------------------------------------
def _two_rank_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)                                                # (as tests/test_dist_gpu.py: gloo transport, both ranks on cuda:0)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    from emdr2_amd.data.index_snapshot import IndexSnapshotWriter
    _, m, ids, index = _paced_index(n=5001)
    assert index.local_rows() == ((0, 2501) if rank == 0 else (2501, 5001))
    writer = IndexSnapshotWriter(index, chunk_rows=600)
    writer.begin(os.path.join(out_dir, "snap.flat"), {"iteration": 6, "refreshes": 1, "mode": "swap"})
    while not writer.pump():
        assert writer._error is None
    it = 0
    while writer.active:
        it += 10
        writer.maybe_finalize(it)                                           # the MIN all-reduce: both ranks leave at the same call
    fresh = _index(min_rows=1 << 30)(embed_size=64, embed_data=None, use_gpu=True)
    fresh.load_flat_snapshot(os.path.join(out_dir, "snap.flat"))
    assert fresh.shard.digest() == index.shard.digest()
    torch.distributed.destroy_process_group()


def test_two_ranks_on_one_gpu_write_one_file_equal_to_the_single_rank_file(tmp_path):
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile
    from emdr2_amd.data.index_snapshot import read_snapshot_meta
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_two_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    _, m, ids, index = _paced_index(n=5001)
    single = str(tmp_path / "single.flat")
    index.save_flat_file(single, {"iteration": 6, "refreshes": 1, "mode": "swap"})
    assert open(single, "rb").read() == open(str(tmp_path / "snap.flat"), "rb").read()
    one, two = read_snapshot_meta(single), read_snapshot_meta(str(tmp_path / "snap.flat"))
    assert (one.pop("world"), two.pop("world")) == (1, 2) and one == two
    assert json.load(open(str(tmp_path / "snap.flat.meta")))["ids_crc32"] == one["ids_crc32"]
    assert np.array_equal(np.asarray(FlatEmbeddingFile(single).rows).view(np.uint16), m.view(np.uint16))
