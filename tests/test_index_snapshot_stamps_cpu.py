"""CPU: generation stamps in index snapshots without a GPU -- the stamp digest's definition (pinned values, properties), the sidecar file,
the protocol of `save_flat_file` / `load_flat_snapshot` over gloo with numpy stand-ins for shards that carry stamps, what stays exactly as
it was for shards without stamps, the refusals, and the argument validation of emdr2_mips_digest_stamps."""
import ctypes
import json
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2 ** 64 - 1


# ---- the definition in plain Python ints (include/emdr2_mips.h: emdr2_mips_digest_stamps) ---------------------------------------------
def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _digest_ints(stamps, row_base=0):
    total, x = 0, 0
    for r, g in enumerate(int(s) for s in stamps):
        h = _mix(_mix(g | (0x47454E53 << 32)) ^ (((row_base + r + 1) * 0x9E3779B97F4A7C15) & M64))
        total, x = (total + h) & M64, x ^ h
    return total, x


# (the values were computed from `_digest_ints` above, the text of the definition, and nothing else)
PINNED = [
    ([0], 0, 0x83d40d4634744454, 0x83d40d4634744454),
    ([0, 1, 2, 6, 2 ** 31 - 1], 0, 0x23fd973165de4e44, 0xa3c5452365e1d206),
    ([0, 1, 2, 6, 2 ** 31 - 1], 1001, 0x723f7a0c350592e1, 0x0869919a15a6afab),
    ([7] * 9, 5, 0x2194b0903845d3f3, 0x7046a069c632237b),
]


@pytest.mark.parametrize("stamps,row_base,want_sum,want_xor", PINNED)
def test_pinned_stamp_digest_values(stamps, row_base, want_sum, want_xor):
    from emdr2_amd.data.emdr2_index import digest_stamps
    assert _digest_ints(stamps, row_base) == (want_sum, want_xor)                          # the text of the definition
    assert digest_stamps(np.array(stamps, dtype=np.uint32), row_base) == (want_sum, want_xor)     # its numpy restatement
    assert digest_stamps(np.array(stamps, dtype=np.int32), row_base) == (want_sum, want_xor)      # (the shard's storage type: same bits)
    assert digest_stamps(np.empty((0,), np.uint32), row_base) == (0, 0)


def _stamps(n, seed=3):
    s = np.random.default_rng(seed).integers(0, 2 ** 31, size=n, dtype=np.int64).astype(np.uint32)
    if n > 1:
        s[0], s[-1] = 0, 2 ** 31 - 1
    return s


def test_stamp_digest_of_a_range_split_combines_and_damage_changes_both_words():
    from emdr2_amd.data.emdr2_index import combine_digests, digest_stamps
    s = _stamps(1000)
    whole = digest_stamps(s)
    assert whole == _digest_ints(s)
    for cut in (0, 1, 129, 999, 1000):
        assert combine_digests([digest_stamps(s[:cut]), digest_stamps(s[cut:], cut)]) == whole
    assert combine_digests([digest_stamps(s[:129], 40), digest_stamps(s[129:], 169)]) == digest_stamps(s, 40) != whole

    def changed(t):
        got = digest_stamps(t)
        return got[0] != whole[0] and got[1] != whole[1]
    a = s.copy(); a[517] ^= 1
    assert changed(a)                                                                      # one stamp changed
    b = s.copy(); b[[3, 700]] = b[[700, 3]]
    assert b[3] != s[3] and changed(b)                                                     # the stamps of two rows swapped
    with pytest.raises(ValueError):
        digest_stamps(s.astype(np.int64))


# ---- the sidecar -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 1000, 1023])
def test_sidecar_round_trip(tmp_path, n):
    from emdr2_amd.data.index_snapshot import StampFile
    s = _stamps(n)
    one, two = str(tmp_path / "w.gen"), str(tmp_path / "c.gen")
    StampFile.write(one, s)
    f = StampFile.create(two, n)
    assert f.n == n
    for lo in range(0, n, 300):                                                            # disjoint slices through separate writable maps
        g = StampFile(two, mode="r+")
        g.stamps[lo:lo + 300] = s[lo:lo + 300]
        g.flush()
    data = open(one, "rb").read()
    assert data == open(two, "rb").read()
    assert len(data) == 24 + 4 * n and data[:8] == b"EMDR2GEN"                            # the documented layout, little-endian
    assert np.array_equal(np.frombuffer(data[8:24], dtype="<u4"), [1, 0, n & 0xffffffff, n >> 32])
    assert np.array_equal(np.frombuffer(data[24:], dtype="<u4"), s)
    back = StampFile(one)
    assert back.n == n and back.stamps.dtype == np.uint32 and np.array_equal(back.stamps, s)
    open(one, "wb").write(b"EMDR2EMB" + data[8:])
    with pytest.raises(ValueError):
        StampFile(one)


# ---- the protocol, numpy shards ----------------------------------------------------------------------------------------------------------
class _NumpyShard(object):
    """Stands in for HipIndexShard: rows and, with `generations`, stamps on the host; the digests from the numpy restatements."""

    def __init__(self, dim, n_rows, row_base, generations):
        self.dim, self.n_rows, self.row_base = dim, n_rows, row_base
        self._rows, self.ids = np.empty((0, dim), np.float16), np.empty((0,), np.int32)
        self.generation = np.zeros(max(n_rows, 1), np.int32) if generations else None

    def append_rows(self, rows, generation=0):
        self._rows = np.array(rows, dtype=np.float16)
        if self.generation is not None:
            self.generation[:] = generation
        return self

    def set_ids(self, ids):
        self.ids = np.array(ids, dtype=np.int32)

    def export_rows(self, local_row, n, out=None):
        return self._rows[local_row:local_row + n]

    def digest(self, local_row=0, n=None):
        from emdr2_amd.data.emdr2_index import digest_rows
        n = self.n_rows - local_row if n is None else n
        return digest_rows(self._rows[local_row:local_row + n], self.row_base + local_row)

    def digest_stamps(self, local_row=0, n=None):
        from emdr2_amd.data.emdr2_index import digest_stamps
        n = self.n_rows - local_row if n is None else n
        return digest_stamps(self.generation[local_row:local_row + n], self.row_base + local_row)

    def set_stamps(self, local_row, stamps):
        self.generation[local_row:local_row + len(stamps)] = np.asarray(stamps).view(np.int32)


def _index_class():
    from emdr2_amd.data import emdr2_index as ei

    class Index(ei.DistributedBruteForceIndex):
        def _make_shard(self, dim, n, base):
            return _NumpyShard(dim, n, base, self.generations)
    return Index


def _data(n, dim=64):
    rng = np.random.default_rng(11)
    return (rng.permutation(n) + 1).astype(np.int32), rng.standard_normal((n, dim)).astype(np.float16)


def _stamped_index(n, generations=True):
    ids, rows = _data(n)
    index = _index_class()(embed_size=64, embed_data=None, use_gpu=True, generations=generations)
    index.add_arrays(ids, rows)
    if generations:
        lo, hi = index.local_rows()
        index.shard.generation[:hi - lo] = _stamps(n)[lo:hi].view(np.int32)
    return index


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, n, out_dir, action):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    path = os.path.join(out_dir, "snap.flat")
    if action in ("save", "save_plain"):
        _stamped_index(n, generations=action == "save").save_flat_file(path, meta={"iteration": 6, "refreshes": 1, "mode": "rolling"})
    else:
        index = _index_class()(embed_size=64, embed_data=None, use_gpu=True, generations=action == "load")
        try:
            meta = index.load_flat_snapshot(path)
            lo, hi = index.local_rows()
            if action == "load":
                assert index.stamps_restored and np.array_equal(index.shard.generation[:hi - lo].view(np.uint32), _stamps(n)[lo:hi])
                assert "stamps" in meta
            else:
                assert not index.stamps_restored and index.shard.generation is None
            verdict = "ok %d" % meta["world"]
        except ValueError as exc:
            verdict = "refused: %s" % exc
        with open(os.path.join(out_dir, "load%d.txt" % rank), "w") as fh:
            fh.write(verdict)
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, n, out_dir, action):
    mp.spawn(_worker, args=(world, _free_port(), n, str(out_dir), action), nprocs=world, join=True)


def _verdicts(tmp_path, world):
    return [open(str(tmp_path / ("load%d.txt" % r))).read() for r in range(world)]


def test_gloo_world_2_save_with_stamps_loads_at_world_1_and_3(tmp_path):
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile, digest_rows, digest_stamps
    from emdr2_amd.data.index_snapshot import StampFile, ids_crc32, read_snapshot_meta, stamps_path
    n = 1001
    ids, rows = _data(n)
    _spawn(2, n, tmp_path, "save")
    path = str(tmp_path / "snap.flat")
    assert sorted(os.listdir(str(tmp_path))) == ["snap.flat", "snap.flat.gen", "snap.flat.meta"]        # no temporary file is left
    single = str(tmp_path / "single.flat")
    FlatEmbeddingFile.write(single, ids, rows)
    assert open(path, "rb").read() == open(single, "rb").read()                            # the data file is what it always was
    os.remove(single)
    assert np.array_equal(StampFile(stamps_path(path)).stamps, _stamps(n))
    meta = read_snapshot_meta(path)
    s, x = digest_rows(rows)
    gs, gx = digest_stamps(_stamps(n))
    assert meta == {"format": 1, "n": n, "dim": 64, "world": 2, "digest_sum": "%016x" % s, "digest_xor": "%016x" % x,
                    "ids_crc32": ids_crc32(ids), "iteration": 6, "refreshes": 1, "mode": "rolling",
                    "stamps": {"digest_sum": "%016x" % gs, "digest_xor": "%016x" % gx}}
    for world in (1, 3):
        _spawn(world, n, tmp_path, "load")
        assert _verdicts(tmp_path, world) == ["ok 2"] * world
    _spawn(2, n, tmp_path, "load_plain")                                                   # an index without stamps ignores the sidecar
    assert _verdicts(tmp_path, 2) == ["ok 2"] * 2
    # one stamp of the sidecar flipped: every rank refuses (the digest is combined over the ranks before it is compared)
    f = StampFile(stamps_path(path), mode="r+")
    f.stamps[900] ^= 0x40
    f.flush(); del f
    _spawn(3, n, tmp_path, "load")
    bad = digest_stamps(StampFile(stamps_path(path)).stamps)
    for verdict in _verdicts(tmp_path, 3):
        assert verdict.startswith("refused: ") and "stamp digest" in verdict
        assert "%016x %016x in HBM" % bad in verdict and "%016x %016x in the meta" % (gs, gx) in verdict
    _spawn(2, n, tmp_path, "load_plain")                                                   # ... and an index without stamps still does not look
    assert _verdicts(tmp_path, 2) == ["ok 2"] * 2


def test_a_save_without_stamps_is_exactly_what_it_was_and_removes_a_stale_sidecar(tmp_path):
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile, digest_rows
    from emdr2_amd.data.index_snapshot import StampFile, ids_crc32, read_snapshot_meta, stamps_path
    n = 1001
    ids, rows = _data(n)
    path = str(tmp_path / "snap.flat")
    _spawn(2, n, tmp_path, "save")                                                         # an earlier snapshot with stamps ...
    assert os.path.exists(stamps_path(path)) and "stamps" in read_snapshot_meta(path)
    _spawn(2, n, tmp_path, "save_plain")                                                   # ... overwritten by one without
    assert sorted(os.listdir(str(tmp_path))) == ["snap.flat", "snap.flat.meta"]
    s, x = digest_rows(rows)
    assert read_snapshot_meta(path) == {"format": 1, "n": n, "dim": 64, "world": 2, "digest_sum": "%016x" % s, "digest_xor": "%016x" % x,
                                        "ids_crc32": ids_crc32(ids), "iteration": 6, "refreshes": 1, "mode": "rolling"}
    single = str(tmp_path / "single.flat")
    FlatEmbeddingFile.write(single, ids, rows)
    assert open(path, "rb").read() == open(single, "rb").read()
    # loaded into an index WITH stamps: today's behaviour, the uniform stamp of the meta's iteration
    index = _index_class()(embed_size=64, embed_data=None, use_gpu=True, generations=True)
    index.load_flat_snapshot(path)
    assert not index.stamps_restored and np.array_equal(index.shard.generation, np.full(n, 6, np.int32))
    # a stale sidecar next to a snapshot whose meta names no stamps is not looked at
    StampFile.write(stamps_path(path), _stamps(5))
    index.load_flat_snapshot(path)
    assert not index.stamps_restored


def test_single_process_round_trip_and_refusals(tmp_path):
    """No process group: one shard.  `read_snapshot_meta` refuses a snapshot whose meta names stamps when the sidecar is missing, truncated
    or holds another n; `load_flat_snapshot` refuses a flipped stamp and names both digests."""
    from emdr2_amd.data.emdr2_index import digest_stamps
    from emdr2_amd.data.index_snapshot import StampFile, read_snapshot_meta, stamps_path
    Index = _index_class()
    n = 300
    index = _stamped_index(n)
    path = str(tmp_path / "snap.flat")
    index.save_flat_file(path, meta={"mode": "rolling", "iteration": 12})
    gen = stamps_path(path)
    want = digest_stamps(_stamps(n))
    assert read_snapshot_meta(path)["stamps"] == {"digest_sum": "%016x" % want[0], "digest_xor": "%016x" % want[1]}
    fresh = Index(embed_size=64, embed_data=None, use_gpu=True, generations=True)
    fresh.load_flat_snapshot(path)
    assert fresh.stamps_restored and np.array_equal(fresh.shard.generation.view(np.uint32), _stamps(n))
    good = open(gen, "rb").read()
    # the sidecar is missing
    os.remove(gen)
    with pytest.raises(ValueError, match="incomplete"):
        read_snapshot_meta(path)
    with pytest.raises(ValueError, match="incomplete"):
        Index(embed_size=64, embed_data=None, use_gpu=True, generations=True).load_flat_snapshot(path)
    # truncated: shorter than its header says
    open(gen, "wb").write(good[:-4])
    with pytest.raises(ValueError, match="shorter"):
        read_snapshot_meta(path)
    open(gen, "wb").write(good[:10])
    with pytest.raises(ValueError):
        read_snapshot_meta(path)
    # a header with another n (and a body that fits it)
    StampFile.write(gen, _stamps(n + 1))
    with pytest.raises(ValueError, match="%d stamps" % (n + 1)):
        read_snapshot_meta(path)
    StampFile.write(gen, _stamps(n - 1))
    with pytest.raises(ValueError, match="%d stamps" % (n - 1)):
        read_snapshot_meta(path)
    # a stamp digest in the meta that is no hex number
    open(gen, "wb").write(good)
    meta_text = open(path + ".meta").read()
    bad = json.loads(meta_text); bad["stamps"]["digest_xor"] = "xyz"
    open(path + ".meta", "w").write(json.dumps(bad))
    with pytest.raises(ValueError):
        read_snapshot_meta(path)
    open(path + ".meta", "w").write(meta_text)
    assert read_snapshot_meta(path)["n"] == n
    # one stamp flipped
    f = StampFile(gen, mode="r+"); f.stamps[17] ^= 1; f.flush(); del f
    flipped = digest_stamps(StampFile(gen).stamps)
    with pytest.raises(ValueError) as info:
        Index(embed_size=64, embed_data=None, use_gpu=True, generations=True).load_flat_snapshot(path)
    assert re.search(r"stamp digest %016x %016x in HBM, %016x %016x in the meta" % (flipped + want), str(info.value))


def test_a_failed_writer_removes_both_part_files(tmp_path):
    from emdr2_amd.data.index_snapshot import IndexSnapshotWriter
    index = _stamped_index(300)
    writer = IndexSnapshotWriter(index, chunk_rows=100)
    writer.begin(str(tmp_path / "snap.flat"), {"mode": "rolling"})
    assert sorted(n.endswith(".gen") for n in os.listdir(str(tmp_path))) == [False, True]                # both part files exist

    class _Unwritable(object):
        def __setitem__(self, key, value):
            raise PermissionError(13, "Permission denied")
    writer._gen_file.stamps = _Unwritable()
    writer.pump()
    with pytest.raises(PermissionError):
        writer.finish()
    assert not writer.active and os.listdir(str(tmp_path)) == []


def test_the_writer_reads_the_stamp_array_at_every_pump(tmp_path):
    """`commit_refresh` swaps `shard.generation` for another array: the chunks behind the swap carry the new array's stamps."""
    from emdr2_amd.data.index_snapshot import IndexSnapshotWriter, StampFile, stamps_path
    index = _stamped_index(300)
    writer = IndexSnapshotWriter(index, chunk_rows=100)
    path = str(tmp_path / "snap.flat")
    writer.begin(path, {"mode": "swap"})
    writer.pump()
    index.shard.generation = np.full(300, 7, np.int32)
    writer.finish()
    assert np.array_equal(StampFile(stamps_path(path)).stamps, np.concatenate([_stamps(300)[:100], np.full(200, 7, np.uint32)]))


# ---- the C entry point refuses bad arguments before any launch ---------------------------------------------------------------------------
def test_digest_stamps_entry_point_validates_arguments_without_a_gpu():
    import __graft_entry__ as g
    from emdr2_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        g.build()
    fn = _native.lib().emdr2_mips_digest_stamps
    one, off4, off2 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4), ctypes.c_void_p(4096 + 2)
    assert fn(one, 1000, 0, 10, 0, None, None) == -1                                       # null digest
    assert fn(one, 1000, 0, 0, 0, None, None) == -1                                        # ... also for an empty range
    assert fn(one, 1000, 0, 10, 0, off4, None) == -1                                       # the 64-bit atomics need an aligned pair
    assert fn(None, 1000, 0, 10, 0, one, None) == -1                                       # null stamps with rows to read
    assert fn(off2, 1000, 0, 10, 0, one, None) == -1                                       # stamps are 4-byte words
    assert fn(one, 1000, -1, 10, 0, one, None) == -1 and fn(one, 1000, 0, -1, 0, one, None) == -1
    assert fn(one, 1000, 991, 10, 0, one, None) == -1 and fn(one, 1000, 1001, 0, 0, one, None) == -1 and fn(one, -1, 0, 0, 0, one, None) == -1
    assert fn(one, 1000, 0, 10, -1, one, None) == -1                                       # row_base < 0
    # an empty range is a no-op, nothing is launched: at the end, over nothing, without stamps, at a 4-byte aligned array
    assert fn(one, 1000, 1000, 0, 0, one, None) == 0 and fn(one, 0, 0, 0, 0, one, None) == 0
    assert fn(None, 0, 0, 0, 5, one, None) == 0 and fn(off4, 1000, 3, 0, 1001, one, None) == 0
