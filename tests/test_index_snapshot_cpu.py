"""CPU: index snapshots without a GPU -- the row digest's definition (pinned values, properties), `FlatEmbeddingFile.create` / `digest`,
the snapshot protocol of `save_flat_file` / `load_flat_snapshot` over gloo with numpy stand-ins for the shards, and the argument
validation of the two new C entry points."""
import ctypes
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = 2 ** 64 - 1


# ---- the definition, restated once more in plain Python ints (slow, a few rows only) ------------------------------------------------
def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _digest_ints(rows, row_base=0):
    total, x = 0, 0
    for r, row in enumerate(rows):
        words = np.ascontiguousarray(row).view("<u4")
        acc = 0
        for j, w in enumerate(words.tolist()):
            acc = (acc + _mix(w | ((j + 1) << 32))) & M64
        g = _mix(acc ^ (((row_base + r + 1) * 0x9E3779B97F4A7C15) & M64))
        total, x = (total + g) & M64, x ^ g
    return total, x


def _ramp():
    return ((np.arange(192, dtype=np.float32).reshape(3, 64)) / 8 - 4).astype(np.float16)


PINNED = [
    (_ramp, 0, 0xd6a8e06be9e8645f, 0xa31aa1eb95a8e515),
    (_ramp, 5, 0xdcdfb522d92f04a1, 0x04185ec52ea8ea5d),
    (lambda: np.zeros((4, 64), np.float16), 0, 0xc084810bf78d309b, 0x4de78fc8099d7dc3),
]


@pytest.mark.parametrize("make,row_base,want_sum,want_xor", PINNED)
def test_pinned_digest_values(tmp_path, make, row_base, want_sum, want_xor):
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile, digest_rows
    rows = make()
    assert _digest_ints(rows, row_base) == (want_sum, want_xor)           # the text of the definition
    assert digest_rows(rows, row_base) == (want_sum, want_xor)             # its numpy restatement
    path = str(tmp_path / "p.flat")
    FlatEmbeddingFile.write(path, np.arange(rows.shape[0], dtype=np.int32), rows)
    assert FlatEmbeddingFile(path).digest(row_base=row_base) == (want_sum, want_xor)


@pytest.fixture(scope="module")
def rows1000():
    return np.random.default_rng(0).standard_normal((1000, 768)).astype(np.float16)


@pytest.fixture(scope="module")
def flat1000(rows1000, tmp_path_factory):
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile
    path = str(tmp_path_factory.mktemp("flat") / "r.flat")
    FlatEmbeddingFile.write(path, np.arange(1000, dtype=np.int32), rows1000)
    return FlatEmbeddingFile(path)


def test_digest_of_a_range_split_combines(flat1000, rows1000):
    from emdr2_amd.data.emdr2_index import combine_digests
    whole = flat1000.digest()
    assert combine_digests([flat1000.digest(0, 129), flat1000.digest(129, 1000)]) == whole
    assert flat1000.digest(0, 1000) == whole and flat1000.digest(7, 7) == (0, 0)
    assert _digest_ints(rows1000[:3]) == flat1000.digest(0, 3)
    assert flat1000.digest(129, 131) == _digest_ints(rows1000[129:131], row_base=129)      # row r of the file is numbered row_base + r
    with pytest.raises(ValueError):
        flat1000.digest(0, 1001)


def test_digest_changes_with_every_kind_of_damage(rows1000):
    from emdr2_amd.data.emdr2_index import digest_rows
    whole = digest_rows(rows1000)

    def changed(rows):
        s, x = digest_rows(rows)
        return s != whole[0] and x != whole[1]

    a = rows1000.copy(); a[[3, 700]] = a[[700, 3]]
    assert not np.array_equal(a[3], rows1000[3]) and changed(a)                            # two rows swapped
    b = rows1000.copy(); b.view(np.uint16)[517, 40] ^= 1
    assert changed(b)                                                                      # one bit flipped
    c = rows1000.copy(); c[5, [10, 11]] = c[5, [11, 10]]
    assert c[5, 10] != rows1000[5, 10] and changed(c)                                      # the two halves of a word swapped
    d = rows1000.copy(); d[5, [10, 11, 20, 21]] = d[5, [20, 21, 10, 11]]
    assert changed(d)                                                                      # two words of a row swapped


def test_create_plus_slice_writes_equal_write(tmp_path, rows1000):
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile
    ids = (np.random.default_rng(1).permutation(1000) + 1).astype(np.int32)
    for n in (1000, 1023, 1, 0):                                                           # ids that end off and on a 4096-byte boundary
        one, two = str(tmp_path / ("w%d.flat" % n)), str(tmp_path / ("c%d.flat" % n))
        rows = np.resize(rows1000, (n, 768)); i = np.resize(ids, n)
        FlatEmbeddingFile.write(one, i, rows)
        f = FlatEmbeddingFile.create(two, n, 768)
        assert (f.n, f.dim) == (n, 768)
        for lo in range(0, n, 300):                                                        # disjoint slices through separate writable maps
            g = FlatEmbeddingFile(two, mode="r+")
            g.rows[lo:lo + 300] = rows[lo:lo + 300]; g.ids[lo:lo + 300] = i[lo:lo + 300]
            g.flush()
        assert open(one, "rb").read() == open(two, "rb").read()


# ---- the protocol over gloo, numpy shards ------------------------------------------------------------------------------------------------
class _NumpyShard(object):
    """Stands in for HipIndexShard: rows on the host, `export_rows` / `digest` from the numpy restatement."""

    def __init__(self, dim, n_rows, row_base):
        self.dim, self.n_rows, self.row_base = dim, n_rows, row_base
        self._rows, self.ids = np.empty((0, dim), np.float16), np.empty((0,), np.int32)

    def append_rows(self, rows):
        self._rows = np.array(rows, dtype=np.float16)
        return self

    def set_ids(self, ids):
        self.ids = np.array(ids, dtype=np.int32)

    def export_rows(self, local_row, n, out=None):
        return self._rows[local_row:local_row + n]

    def digest(self, local_row=0, n=None):
        from emdr2_amd.data.emdr2_index import digest_rows
        n = self.n_rows - local_row if n is None else n
        return digest_rows(self._rows[local_row:local_row + n], self.row_base + local_row)


def _index_class():
    from emdr2_amd.data import emdr2_index as ei

    class Index(ei.DistributedBruteForceIndex):
        def _make_shard(self, dim, n, base):
            return _NumpyShard(dim, n, base)
    return Index


def _data(n, dim=64):
    rng = np.random.default_rng(11)
    return (rng.permutation(n) + 1).astype(np.int32), rng.standard_normal((n, dim)).astype(np.float16)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _snapshot_worker(rank, world, port, n, out_dir, action):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    ids, rows = _data(n)
    index = _index_class()(embed_size=64, embed_data=None, use_gpu=True)
    path = os.path.join(out_dir, "snap.flat")
    if action == "save":
        index.add_arrays(ids, rows)
        index.save_flat_file(path, meta={"iteration": 6, "refreshes": 1, "mode": "swap"})
    else:
        try:
            meta = index.load_flat_snapshot(path)
            verdict = "ok %d" % meta["world"]
            lo, hi = index.local_rows()
            assert np.array_equal(index.shard._rows.view(np.uint16), rows[lo:hi].view(np.uint16)) and np.array_equal(index.shard.ids, ids[lo:hi])
        except ValueError as exc:
            verdict = "refused: %s" % exc
        with open(os.path.join(out_dir, "load%d.txt" % rank), "w") as fh:
            fh.write(verdict)
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, n, out_dir, action):
    mp.spawn(_snapshot_worker, args=(world, _free_port(), n, str(out_dir), action), nprocs=world, join=True)


@pytest.mark.parametrize("world,other", [(2, 3), (3, 2)])
def test_gloo_save_equals_single_rank_file_and_loads_at_another_world_size(tmp_path, world, other):
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile, digest_rows
    from emdr2_amd.data.index_snapshot import ids_crc32, read_snapshot_meta
    n = 1001
    ids, rows = _data(n)
    single = str(tmp_path / "single.flat")
    FlatEmbeddingFile.write(single, ids, rows)
    _spawn(world, n, tmp_path, "save")
    path = str(tmp_path / "snap.flat")
    assert open(path, "rb").read() == open(single, "rb").read()
    assert sorted(os.listdir(str(tmp_path))) == ["single.flat", "snap.flat", "snap.flat.meta"]         # no temporary file is left
    meta = read_snapshot_meta(path)
    s, x = digest_rows(rows)
    assert meta == {"format": 1, "n": n, "dim": 64, "world": world, "digest_sum": "%016x" % s, "digest_xor": "%016x" % x,
                    "ids_crc32": ids_crc32(ids), "iteration": 6, "refreshes": 1, "mode": "swap"}
    _spawn(other, n, tmp_path, "load")
    assert [open(str(tmp_path / ("load%d.txt" % r))).read() for r in range(other)] == ["ok %d" % world] * other
    # one byte of the rows flipped: every rank refuses (the digest is combined over the ranks before it is compared)
    f = FlatEmbeddingFile(path, mode="r+")
    f.rows.view(np.uint8)[900, 17] ^= 0x40
    f.flush(); del f
    _spawn(other, n, tmp_path, "load")
    for r in range(other):
        assert open(str(tmp_path / ("load%d.txt" % r))).read().startswith("refused: "), r


def test_single_process_save_load_and_incomplete_snapshots(tmp_path):
    """No process group: one shard.  A data file without a meta is refused as a snapshot; so are damaged ids and a meta that disagrees with
    the file's header; an overwrite replaces file and meta; the world-1 file equals the world-2 one by construction (`write`)."""
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile
    from emdr2_amd.data.index_snapshot import meta_path, read_snapshot_meta
    Index = _index_class()
    ids, rows = _data(300)
    index = Index(embed_size=64, embed_data=None, use_gpu=True)
    index.add_arrays(ids, rows)
    path = str(tmp_path / "snap.flat")
    index.save_flat_file(path, meta={"mode": "build"})
    single = str(tmp_path / "single.flat")
    FlatEmbeddingFile.write(single, ids, rows)
    assert open(path, "rb").read() == open(single, "rb").read()
    assert read_snapshot_meta(path)["mode"] == "build" and read_snapshot_meta(path)["world"] == 1
    fresh = Index(embed_size=64, embed_data=None, use_gpu=True)
    assert fresh.load_flat_snapshot(path)["n"] == 300 and np.array_equal(fresh.shard.ids, ids)
    # overwrite with other rows: one file, a new meta
    index.add_arrays(ids[:200], rows[:200])
    index.save_flat_file(path, meta={"mode": "swap", "iteration": 12})
    assert read_snapshot_meta(path)["n"] == 200 and read_snapshot_meta(path)["iteration"] == 12
    meta_text = open(meta_path(path)).read()
    # a data file alone is an incomplete snapshot
    os.remove(meta_path(path))
    with pytest.raises(ValueError, match="incomplete"):
        read_snapshot_meta(path)
    with pytest.raises(ValueError, match="incomplete"):
        Index(embed_size=64, embed_data=None, use_gpu=True).load_flat_snapshot(path)
    with pytest.raises(FileNotFoundError):
        read_snapshot_meta(str(tmp_path / "nothing.flat"))
    # a meta whose n disagrees with the header; damaged ids
    bad = json.loads(meta_text); bad["n"] = 201
    open(meta_path(path), "w").write(json.dumps(bad))
    with pytest.raises(ValueError):
        read_snapshot_meta(path)
    open(meta_path(path), "w").write(meta_text)
    f = FlatEmbeddingFile(path, mode="r+"); f.ids[5] += 1; f.flush(); del f
    with pytest.raises(ValueError, match="ids"):
        Index(embed_size=64, embed_data=None, use_gpu=True).load_flat_snapshot(path)
    with pytest.raises(ValueError):
        Index(embed_size=128, embed_data=None, use_gpu=True).load_flat_snapshot(path)


def test_a_failed_begin_and_a_failed_writer_raise(tmp_path):
    """A snapshot into a directory that does not exist fails in `begin` (rank 0 creates the file there); an error of the background
    thread surfaces from `finish()`, and neither leaves a file under the snapshot's name."""
    from emdr2_amd.data.index_snapshot import IndexSnapshotWriter
    ids, rows = _data(300)
    index = _index_class()(embed_size=64, embed_data=None, use_gpu=True)
    index.add_arrays(ids, rows)
    with pytest.raises(OSError):
        index.save_flat_file(str(tmp_path / "missing" / "snap.flat"))
    writer = IndexSnapshotWriter(index, chunk_rows=100)
    path = str(tmp_path / "snap.flat")
    writer.begin(path, {"mode": "swap"})

    class _Unwritable(object):
        def __setitem__(self, key, value):
            raise PermissionError(13, "Permission denied")
    writer._file.rows = _Unwritable()
    writer.pump()
    with pytest.raises(PermissionError):
        writer.finish()
    assert not writer.active and os.listdir(str(tmp_path)) == []


def test_paced_chunk_covers_the_shard_in_half_an_interval():
    from emdr2_amd.data.index_snapshot import IndexSnapshotWriter, SNAPSHOT_ROWS
    from emdr2_amd.data.emdr2_index import _UPLOAD_ROWS
    assert SNAPSHOT_ROWS <= _UPLOAD_ROWS
    for n, interval in ((2626916, 500), (20000, 500), (1000, 6), (5, 500), (0, 500)):
        chunk = IndexSnapshotWriter.paced_chunk_rows(n, interval)
        assert 1 <= chunk <= SNAPSHOT_ROWS and chunk * max(1, interval // 2) >= n


# ---- the C entry points refuse bad arguments before any launch ---------------------------------------------------------------------------
def test_export_and_digest_entry_points_validate_arguments_without_a_gpu():
    import __graft_entry__ as g
    from emdr2_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        g.build()
    lib = _native.lib()
    one, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)
    for fn, tail in ((lib.emdr2_mips_export_rows, (one, None)), (lib.emdr2_mips_digest_rows, (0, one, None))):
        assert fn(None, 1000, 768, 0, 10, *tail) == -1                                     # null image
        assert fn(one, 1000, 100, 0, 10, *tail) == -1 and fn(one, 1000, 32, 0, 10, *tail) == -1 and fn(one, 1000, 8224, 0, 10, *tail) == -1
        assert fn(one, 1000, 768, -1, 10, *tail) == -1 and fn(one, 1000, 768, 0, -1, *tail) == -1
        assert fn(one, 1000, 768, 991, 10, *tail) == -1 and fn(one, 1000, 768, 1001, 0, *tail) == -1 and fn(one, -1, 768, 0, 0, *tail) == -1
        assert fn(one, 1000, 768, 1000, 0, *tail) == 0 and fn(one, 0, 768, 0, 0, *tail) == 0     # an empty range: a no-op, nothing launched
    assert lib.emdr2_mips_export_rows(one, 1000, 768, 0, 10, None, None) == -1
    assert lib.emdr2_mips_digest_rows(one, 1000, 768, 0, 10, 0, None, None) == -1
    assert lib.emdr2_mips_digest_rows(one, 1000, 768, 0, 10, 0, odd, None) == -1              # the 64-bit atomics need an aligned pair
