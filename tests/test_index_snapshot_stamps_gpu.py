"""GPU: generation stamps in index snapshots -- emdr2_mips_digest_stamps against its numpy restatement bit for bit (unaligned heads and
tails, a 4-byte aligned array, the grid-stride body), the shard's stamp accessors, the save / load round trip of stamped shards, the paced
writer under stamped updates on both sides of its cursor (a row and its stamp leave the device at the same stream point), a swap refresh
between pumps, and two gloo ranks on the one GPU."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests.test_index_generations_cpu import apply_list, apply_range, stats_words
from tests.test_index_oldest_cpu import oldest_rows_reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2 ** 64 - 1
GEN_TOP = 2 ** 31 - 1


def _stamps(n, seed=3):
    """random over the full 31 bits, 0 and 2^31 - 1 among them"""
    s = np.random.default_rng(seed + n).integers(0, 2 ** 31, size=n, dtype=np.int64).astype(np.uint32)
    s[0] = 0
    s[-1] = GEN_TOP
    if n > 4:
        s[3] = GEN_TOP; s[4] = 0
    return s


def _pair(acc):
    s, x = acc.tolist()
    return s & M64, x & M64


# ---- the kernel ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000, 70001])
def test_device_stamp_digest_equals_the_numpy_restatement(n, shift):
    """`shift`: the stamp array starts `shift` words behind a 16-byte boundary (it is only promised 4-byte alignment), so with the range
    starts 0, 1, 3 and 257 the scalar head takes every length from 0 to 3 and so does the tail."""
    from emdr2_amd import _native
    from emdr2_amd.data.emdr2_index import combine_digests, digest_stamps
    lib = _native.lib()
    host = _stamps(n)
    store = torch.zeros(n + 8, dtype=torch.int32, device="cuda")
    assert store.data_ptr() % 16 == 0
    gen = store[shift:shift + n]
    gen.copy_(torch.from_numpy(host.view(np.int32).copy()))
    acc = torch.zeros(2, dtype=torch.int64, device="cuda")

    def device(lo, cnt, row_base, into=None):
        a = acc.zero_() if into is None else into
        _native.check(lib.emdr2_mips_digest_stamps(gen.data_ptr(), n, lo, cnt, row_base, a.data_ptr(), _native.stream_ptr()), "digest_stamps")
        return _pair(a)

    for row_base in (0, 1001):
        for lo in (0, 1, 3, 257):
            for hi in (n, n - 1):
                if lo > hi:
                    continue
                assert device(lo, hi - lo, row_base) == digest_stamps(host[lo:hi], row_base + lo), (n, shift, row_base, lo, hi)
    # n_chunk == 0 leaves the accumulator alone; two ranges folded into one accumulator are the whole
    whole = digest_stamps(host, 1001)
    two = torch.zeros(2, dtype=torch.int64, device="cuda")
    cut = min(n, 129)
    device(0, cut, 1001, into=two)
    first = _pair(two)
    assert device(cut, 0, 1001, into=two) == first == digest_stamps(host[:cut], 1001)
    assert device(cut, n - cut, 1001, into=two) == whole
    assert combine_digests([first, digest_stamps(host[cut:], 1001 + cut)]) == whole


# ---- the shard's accessors -------------------------------------------------------------------------------------------------------------
def _index(dim, generations=True):
    from emdr2_amd.data import emdr2_index as ei

    class Index(ei.DistributedBruteForceIndex):
        def _make_shard(self, dim, n, base):
            return ei.HipIndexShard(dim, n, base, shadow_min_rows=1, generations=self.generations)
    return Index(embed_size=dim, embed_data=None, use_gpu=True, generations=generations)


def _filled(n, dim, seed, generations=True):
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((n, dim)).astype(np.float16)
    ids = (rng.permutation(n) + 1).astype(np.int32)
    index = _index(dim, generations)
    index.add_arrays(ids, m)
    return rng, m, ids, index


def test_shard_stamp_accessors():
    from emdr2_amd.data.emdr2_index import digest_stamps
    n = 1000
    _, m, ids, index = _filled(n, 64, 1)
    sh = index.shard
    s = _stamps(n)
    assert sh.digest_stamps() == digest_stamps(np.zeros(n, np.uint32))                     # loaded rows are stamped 0
    sh.set_stamps(0, s)
    assert np.array_equal(sh.generation.cpu().numpy().view(np.uint32), s)
    sh.set_stamps(129, s[:5].view(np.int32))                                               # the storage type; a range inside the shard
    s[129:134] = s[:5]
    assert np.array_equal(sh.export_stamps(0, n).cpu().numpy().view(np.uint32), s)
    assert sh.digest_stamps() == digest_stamps(s) and sh.digest_stamps(3, 254) == digest_stamps(s[3:257], 3)
    assert sh.digest_stamps(n, 0) == (0, 0) and sh.export_stamps(n, 0).shape == (0,)
    out = torch.full((n + 3,), 7, dtype=torch.int32, device="cuda")                        # a caller's buffer: only its first words are written
    got = sh.export_stamps(257, 700, out=out)
    assert got.data_ptr() == out.data_ptr() and np.array_equal(got.cpu().numpy().view(np.uint32), s[257:957]) and bool((out[700:] == 7).all())
    acc = torch.zeros(2, dtype=torch.int64, device="cuda")
    assert sh.digest_stamps_into(acc, 0, 100) is acc and _pair(sh.digest_stamps_into(acc, 100)) == digest_stamps(s)
    for call in (lambda: sh.set_stamps(0, np.array([2 ** 31], np.uint32)), lambda: sh.set_stamps(0, np.array([-1], np.int32)),
                 lambda: sh.set_stamps(0, np.zeros(3, np.int64)), lambda: sh.set_stamps(n - 1, np.zeros(2, np.uint32)),
                 lambda: sh.set_stamps(-1, np.zeros(2, np.uint32)), lambda: sh.export_stamps(0, n + 1), lambda: sh.digest_stamps(1, n),
                 lambda: sh.export_stamps(0, n, out=torch.empty(n, dtype=torch.int64, device="cuda")),
                 lambda: sh.digest_stamps_into(torch.zeros(2, dtype=torch.int32, device="cuda"))):
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(sh.generation.cpu().numpy().view(np.uint32), s)                  # a refused call changed nothing
    plain = _filled(300, 64, 2, generations=False)[3].shard
    for call in (lambda: plain.export_stamps(0, 1), plain.digest_stamps, lambda: plain.set_stamps(0, np.zeros(1, np.uint32))):
        with pytest.raises(ValueError):
            call()


# ---- round trip --------------------------------------------------------------------------------------------------------------------------
# 1,000 x 64: no shadow, padding to 1,024.  2,049 x 768: a shadow is asked for (shadow_min_rows = 1) and the last 256-row block holds one row;
# the search plan gives no shard below 8,193 rows an int8 segment, so the shape that does SEAL a shadow, 8,193 x 768 with the same one-row
# last block, is run as well.
@pytest.mark.parametrize("n,dim,shadow", [(1000, 64, False), (2049, 768, False), (8193, 768, True)])
def test_round_trip_restores_every_stamp(tmp_path, n, dim, shadow):
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile, digest_stamps, generation_result
    from emdr2_amd.data.index_snapshot import StampFile, read_snapshot_meta, stamps_path
    _, m, ids, a = _filled(n, dim, n)
    assert (a.shard._shadow is not None) == shadow and a.shard._want_shadow == shadow
    s = _stamps(n)
    a.shard.set_stamps(0, s)
    path = str(tmp_path / "snap.flat")
    a.save_flat_file(path, meta={"iteration": 40, "refreshes": 2, "mode": "rolling"})
    assert sorted(os.listdir(str(tmp_path))) == ["snap.flat", "snap.flat.gen", "snap.flat.meta"]
    assert np.array_equal(StampFile(stamps_path(path)).stamps, s)
    assert np.array_equal(np.asarray(FlatEmbeddingFile(path).rows).view(np.uint16), m.view(np.uint16))
    meta = read_snapshot_meta(path)
    gs, gx = digest_stamps(s)
    assert meta["stamps"] == {"digest_sum": "%016x" % gs, "digest_xor": "%016x" % gx} and meta["format"] == 1
    b = _index(dim)
    assert b.load_flat_snapshot(path) == meta and b.stamps_restored
    now, below = 2 ** 31, 2 ** 30
    torch.cuda.synchronize()
    assert torch.equal(a.shard.generation[:n], b.shard.generation[:n])
    assert np.array_equal(b.shard.generation.cpu().numpy()[:n].view(np.uint32), s)
    assert a.generation_stats(now) == b.generation_stats(now) == generation_result(stats_words(s, now))
    (ra, ia), (rb, ib) = a.oldest_rows(300, below), b.oldest_rows(300, below)
    want_rows, want_info = oldest_rows_reference(s, 300, below)
    assert torch.equal(ra, rb) and torch.equal(ia, ib)
    assert np.array_equal(rb.cpu().numpy(), want_rows) and [w & M64 for w in ib.tolist()] == want_info
    assert not np.array_equal(want_rows, np.arange(300))                                   # (what uniform stamps would select)
    assert a.shard.digest() == b.shard.digest() == (int(meta["digest_sum"], 16), int(meta["digest_xor"], 16))
    assert a.shard.digest_stamps() == b.shard.digest_stamps() == (gs, gx)
    assert torch.equal(a.shard.tiled, b.shard.tiled) and (b.shard._shadow is not None) == shadow
    # an index without generations loads it and has no stamps
    c = _index(dim, generations=False)
    assert c.load_flat_snapshot(path) == meta and c.shard.generation is None and not c.stamps_restored
    assert c.shard.digest() == a.shard.digest()
    # one stamp of the sidecar flipped: the device digest of the stamps no longer matches the meta
    f = StampFile(stamps_path(path), mode="r+"); f.stamps[n - 1] ^= 1; f.flush(); del f
    d = _index(dim)
    with pytest.raises(ValueError, match="stamp digest .* in HBM, %016x %016x in the meta" % (gs, gx)):
        d.load_flat_snapshot(path)


def test_a_snapshot_without_stamps_is_what_it_was(tmp_path):
    """From an index without stamps: no sidecar, no `stamps` key, a stale sidecar removed; loaded into an index with stamps every row gets
    the meta's iteration."""
    from emdr2_amd.data.index_snapshot import StampFile, read_snapshot_meta, stamps_path
    n = 1000
    _, m, ids, a = _filled(n, 64, 5, generations=False)
    path = str(tmp_path / "snap.flat")
    StampFile.write(stamps_path(path), _stamps(n))
    a.save_flat_file(path, meta={"iteration": 40, "mode": "swap"})
    assert sorted(os.listdir(str(tmp_path))) == ["snap.flat", "snap.flat.meta"]
    assert sorted(read_snapshot_meta(path)) == ["digest_sum", "digest_xor", "dim", "format", "ids_crc32", "iteration", "mode", "n", "world"]
    b = _index(64)
    b.load_flat_snapshot(path)
    assert not b.stamps_restored and bool((b.shard.generation == 40).all())


# ---- the paced writer: a row and its stamp leave the device at the same stream point ---------------------------------------------------
def _marked(rng, k, dim, g):
    """k fresh rows that carry fp16(g) in element 0"""
    new = rng.standard_normal((k, dim)).astype(np.float16)
    new[:, 0] = np.float16(g)
    return new


def _dev(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def test_torn_export_keeps_every_row_with_its_own_stamp(tmp_path):
    """2,000 x 64, 256 rows per pump.  Every row written at generation g carries fp16(g) in element 0 (g <= 2,048: exact).  Before each
    pump, with the cursor at c: a stamped range update across c, a scattered stamped update with ids on both sides of c, and a newest-wins
    range update across c that leaves the scattered rows alone.  Rows behind c were exported before: the file keeps their old row AND
    their old stamp.  Rows at or ahead of c are exported afterwards: the file holds the new row AND the new stamp."""
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile, digest_stamps
    from emdr2_amd.data.index_snapshot import IndexSnapshotWriter, StampFile, read_snapshot_meta, stamps_path
    n, dim = 2000, 64
    rng = np.random.default_rng(9)
    first = _marked(rng, n, dim, 1)
    index = _index(dim)
    index._load_generation = 1
    index.add_arrays(np.arange(1, n + 1, dtype=np.int32), first)
    sh = index.shard
    live, live_stamps = first.copy(), np.full(n, 1, dtype=np.int64)
    want, want_stamps = first.copy(), np.full(n, 1, dtype=np.int64)
    writer = IndexSnapshotWriter(index, chunk_rows=256)
    path = str(tmp_path / "snap.flat")
    writer.begin(path, {"iteration": 40, "refreshes": 2, "mode": "rolling"})
    behind = ahead = kept_total = pumps = 0
    g = 10
    while True:
        c = writer._cursor
        g += 3
        assert g + 1 <= 2048
        # (a) a stamped range update that crosses the cursor
        lo, hi = max(c - 50, 0), min(c + 50, n)
        new = _marked(rng, hi - lo, dim, g)
        sh.update_rows(lo, _dev(new, np.float16), generation=g)
        apply_range(live, live_stamps, lo, new, g, False)
        apply_range(want, want_stamps, max(lo, c), new[max(lo, c) - lo:], g, False)
        # (b) a scattered stamped update, ids on both sides of the cursor, one generation ahead
        pool = np.arange(max(c - 200, 0), min(c + 200, n))
        ids = rng.choice(pool, size=min(60, pool.size), replace=False).astype(np.int64)
        new = _marked(rng, ids.size, dim, g + 1)
        sh.update_rows_at(_dev(ids, np.int64), _dev(new, np.float16), generation=g + 1)
        apply_list(live, live_stamps, ids, new, g + 1, False)
        apply_list(want, want_stamps, ids[ids >= c], new[ids >= c], g + 1, False)
        behind += int((ids < c).sum()); ahead += int((ids >= c).sum())
        # (c) a newest-wins range update across the cursor: the rows (b) has just stamped g + 1 stay as they are
        lo, hi = max(c - 100, 0), min(c + 100, n)
        new = _marked(rng, hi - lo, dim, g)
        sh.update_rows(lo, _dev(new, np.float16), generation=g, newest_wins=True)
        kept = apply_range(live, live_stamps, lo, new, g, True)
        apply_range(want, want_stamps, max(lo, c), new[max(lo, c) - lo:], g, True)
        assert sh.kept_newer() == kept
        kept_total += kept
        moved = writer._cursor
        assert writer._error is None
        done = writer.pump()
        pumps += writer._cursor != moved
        if done:
            break
        if writer._cursor == moved:                                         # both buffers busy: pump() did nothing and did not block
            torch.cuda.synchronize()
    writer.finish()
    assert pumps == 8 and behind > 100 and ahead > 100 and kept_total > 50
    flat, side = FlatEmbeddingFile(path), StampFile(stamps_path(path))
    rows, stamps = np.asarray(flat.rows), np.asarray(side.stamps).astype(np.int64)
    assert np.array_equal(rows[:, 0].astype(np.float64), stamps.astype(np.float64))        # every row of the file with its own stamp
    assert np.array_equal(stamps, want_stamps) and np.array_equal(rows.view(np.uint16), want.view(np.uint16))
    # both sides of the cursor were hit: rows whose file pair is the OLD one (the live index has moved on), rows whose pair is new
    stale = stamps != live_stamps
    assert stale.sum() > 100 and (stamps != 1).sum() > 500
    assert np.array_equal(sh.generation.cpu().numpy()[:n].astype(np.int64), live_stamps)
    assert np.array_equal(sh.export_rows(0, n).cpu().numpy().view(np.uint16), live.view(np.uint16))
    meta = read_snapshot_meta(path)
    assert (int(meta["digest_sum"], 16), int(meta["digest_xor"], 16)) == flat.digest()
    assert (int(meta["stamps"]["digest_sum"], 16), int(meta["stamps"]["digest_xor"], 16)) == digest_stamps(np.asarray(side.stamps))
    assert sorted(os.listdir(str(tmp_path))) == ["snap.flat", "snap.flat.gen", "snap.flat.meta"]


def test_a_swap_refresh_between_pumps_is_followed(tmp_path):
    """`commit_refresh` swaps `shard.generation` for the spare array: the writer reads the attribute at every pump, so the chunks behind
    the swap carry the new image's rows and stamps."""
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile, digest_stamps
    from emdr2_amd.data.index_snapshot import IndexSnapshotWriter, StampFile, read_snapshot_meta, stamps_path
    n, dim = 2000, 64
    rng, m, ids, index = _filled(n, dim, 21)
    s = _stamps(n)
    s[s == 7] = 8
    index.shard.set_stamps(0, s)
    writer = IndexSnapshotWriter(index, chunk_rows=256)
    path = str(tmp_path / "snap.flat")
    writer.begin(path, {"iteration": 7, "refreshes": 1, "mode": "swap"})
    assert writer.pump() is False and writer.pump() is False and writer._cursor == 512
    new = rng.standard_normal((n, dim)).astype(np.float16)
    old_array = index.shard.generation
    index.begin_refresh(generation=7)
    index.refresh_rows(0, _dev(new, np.float16))
    index.commit_refresh()
    assert index.shard.generation is not old_array
    writer.finish()
    want = np.concatenate([s[:512], np.full(n - 512, 7, np.uint32)])
    side, flat = StampFile(stamps_path(path)), FlatEmbeddingFile(path)
    assert np.array_equal(side.stamps, want)
    assert np.array_equal(np.asarray(flat.rows).view(np.uint16), np.concatenate([m[:512], new[512:]]).view(np.uint16))
    meta = read_snapshot_meta(path)
    assert (int(meta["stamps"]["digest_sum"], 16), int(meta["stamps"]["digest_xor"], 16)) == digest_stamps(want)
    assert (int(meta["digest_sum"], 16), int(meta["digest_xor"], 16)) == flat.digest()


# ---- two ranks on one GPU ----------------------------------------------------------------------------------------------------------------
def _rank_stamps(n):
    """stamps that differ per rank: rank 0's rows (the first 1,001 of 2,001) are old, rank 1's young, both random"""
    rng = np.random.default_rng(17)
    s = np.concatenate([rng.integers(0, 500, 1001), rng.integers(2 ** 30, 2 ** 31, n - 1001)]).astype(np.uint32)
    s[0], s[-1] = 0, GEN_TOP
    return s


def _two_rank_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)                                                # (as tests/test_dist_gpu.py: gloo transport, both ranks on cuda:0)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    n = 2001
    _, m, ids, index = _filled(n, 64, 23)
    lo, hi = index.local_rows()
    assert (lo, hi) == ((0, 1001) if rank == 0 else (1001, 2001))
    index.shard.set_stamps(0, _rank_stamps(n)[lo:hi])
    index.save_flat_file(os.path.join(out_dir, "snap.flat"), {"iteration": 6, "refreshes": 1, "mode": "rolling"})
    fresh = _index(64)
    fresh.load_flat_snapshot(os.path.join(out_dir, "snap.flat"))
    assert fresh.stamps_restored and torch.equal(fresh.shard.generation, index.shard.generation)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


def test_two_ranks_on_one_gpu_save_stamps_that_one_rank_loads(tmp_path):
    from emdr2_amd.data.emdr2_index import digest_stamps
    from emdr2_amd.data.index_snapshot import StampFile, read_snapshot_meta, stamps_path
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_two_rank_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    n = 2001
    path = str(tmp_path / "snap.flat")
    want = _rank_stamps(n)
    meta = read_snapshot_meta(path)
    assert meta["world"] == 2 and np.array_equal(StampFile(stamps_path(path)).stamps, want)
    gs, gx = digest_stamps(want)
    assert meta["stamps"] == {"digest_sum": "%016x" % gs, "digest_xor": "%016x" % gx}
    one = _index(64)
    one.load_flat_snapshot(path)                                            # world 1
    assert one.stamps_restored and np.array_equal(one.shard.generation.cpu().numpy().view(np.uint32), want)
    f = StampFile(stamps_path(path), mode="r+"); f.stamps[1500] ^= 2; f.flush(); del f
    with pytest.raises(ValueError, match="stamp digest"):
        one.load_flat_snapshot(path)
