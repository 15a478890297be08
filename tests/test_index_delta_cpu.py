"""CPU: incremental index snapshots (data/index_snapshot.py) without a GPU -- the numpy restatement of the row keys pinned on
the existing host digests and on literals, the delta file and its meta (round trips and refusals), the protocol on gloo ranks over numpy
stand-ins for the shard (a world of 2 writes, worlds of 1 and 3 read), and the argument checks of the three C entry points."""
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


def _fold(keys):
    return int(keys.sum(dtype=np.uint64)), int(np.bitwise_xor.reduce(keys)) if keys.size else 0


# ---- the keys ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim,base", [(1, 64, 0), (257, 64, 1001), (1000, 96, 7), (70000, 64, 3)])
def test_row_keys_are_the_terms_of_the_host_digests(n, dim, base):
    from emdr2_amd.data.emdr2_index import digest_rows, digest_stamps, row_keys
    rng = np.random.default_rng(n)
    rows = rng.standard_normal((n, dim)).astype(np.float16)
    stamps = rng.integers(0, 2 ** 31, size=n, dtype=np.int64).astype(np.uint32)
    plain = row_keys(rows, None, base)
    assert plain.dtype == np.uint64 and plain.shape == (n,) and _fold(plain) == digest_rows(rows, base)
    with np.errstate(over="ignore"):
        h = row_keys(rows, stamps, base) - plain                                           # mod 2^64
    assert _fold(h) == digest_stamps(stamps, base)
    assert np.array_equal(row_keys(rows, stamps.view(np.int32), base), row_keys(rows, stamps, base))   # the storage type of the stamps
    # a key depends on its own row, stamp and number alone
    cut = n // 2
    assert np.array_equal(row_keys(rows[cut:], stamps[cut:], base + cut), row_keys(rows, stamps, base)[cut:])
    if n > 1:
        assert not np.array_equal(row_keys(rows, None, base + 1)[:-1], plain[1:])          # the number enters


def test_row_keys_literals_and_refusals():
    from emdr2_amd.data.emdr2_index import row_keys
    rows = (np.arange(3 * 64, dtype=np.float32).reshape(3, 64) / 16).astype(np.float16)
    stamps = np.array([0, 5, 2 ** 31 - 1], np.uint32)
    assert row_keys(rows, None, 0).tolist() == [0xD7D346B4C72D5481, 0x22C17EAB7479EE71, 0xA10C5A8B56EA05E4]
    assert row_keys(rows, stamps, 0).tolist() == [0x5BA753FAFBA198D5, 0xF67CFF1F82A411E7, 0x5B057EC7E5DDCB37]
    assert row_keys(rows, stamps, 1000)[2] == 0xBA8572A65F6D5305
    for call in (lambda: row_keys(rows.astype(np.float32)), lambda: row_keys(rows[0]), lambda: row_keys(rows, stamps[:2]),
                 lambda: row_keys(rows, stamps.astype(np.int64))):
        with pytest.raises(ValueError):
            call()
    assert row_keys(rows[:0], stamps[:0]).shape == (0,)


# ---- the delta file and its meta -------------------------------------------------------------------------------------------------------------
def _base_meta(n, dim, stamped):
    meta = {"format": 1, "n": n, "dim": dim, "world": 1, "digest_sum": "%016x" % 11, "digest_xor": "%016x" % 12, "ids_crc32": 0}
    if stamped:
        meta["stamps"] = {"digest_sum": "%016x" % 13, "digest_xor": "%016x" % 14}
    return meta


def _write_delta(path, n, dim, m, stamped, base_meta, iteration=9):
    """a delta of m rows next to `path`, written with the module's own pieces -> (rows, stamps, data, meta)"""
    from emdr2_amd.data import index_snapshot as snap
    rng = np.random.default_rng(m + dim)
    rows = np.sort(rng.choice(n, size=m, replace=False)).astype(np.int64)
    data = rng.standard_normal((m, dim)).astype(np.float16)
    stamps = rng.integers(0, 2 ** 31, size=m, dtype=np.int64).astype(np.uint32) if stamped else None
    flat = snap.DeltaFile.create(snap.delta_path(path), m, dim, stamped)
    snap._write_slice(flat, 0, rows, stamps, data, False)
    del flat
    meta = {"format": 1, "m": m, "n": n, "dim": dim, "world": 1, "iteration": iteration, "base": snap.base_of(base_meta),
            "result": snap.IndexSnapshotWriter._digest_meta((1, 2), (3, 4) if stamped else None), "rows_crc32": snap.rows_crc32(rows)}
    with open(snap.delta_meta_path(path), "w") as fh:
        json.dump(meta, fh)
    return rows, stamps, data, meta


@pytest.mark.parametrize("dim", [64, 768])
@pytest.mark.parametrize("stamped", [False, True])
@pytest.mark.parametrize("m", [0, 1, 1000])
def test_delta_file_round_trip(tmp_path, m, stamped, dim):
    from emdr2_amd.data import index_snapshot as snap
    n = 5000
    path = str(tmp_path / "snap.flat")
    base = _base_meta(n, dim, stamped)
    rows, stamps, data, meta = _write_delta(path, n, dim, m, stamped, base)
    raw = open(snap.delta_path(path), "rb").read()
    # the documented layout, little-endian, every section 16-byte aligned
    assert raw[:8] == b"EMDR2DLT" and np.frombuffer(raw[8:32], "<u4").tolist() == [1, int(stamped), m, 0, dim, 0]
    at = 32
    assert np.array_equal(np.frombuffer(raw[at:at + 8 * m], "<i8"), rows)
    at = (at + 8 * m + 15) // 16 * 16
    if stamped:
        assert np.array_equal(np.frombuffer(raw[at:at + 4 * m], "<u4"), stamps)
        at = (at + 4 * m + 15) // 16 * 16
    assert np.array_equal(np.frombuffer(raw[at:at + 2 * m * dim], "<u2"), data.view(np.uint16).ravel()) and len(raw) == at + 2 * m * dim
    back = snap.DeltaFile(snap.delta_path(path))
    assert (back.m, back.dim, back.stamped) == (m, dim, stamped)
    assert np.array_equal(back.rows, rows) and np.array_equal(back.data.view(np.uint16), data.view(np.uint16))
    assert (back.stamps is None) == (not stamped) and (not stamped or np.array_equal(back.stamps, stamps))
    assert snap.read_delta_meta(path, base) == meta


def test_delta_refusals(tmp_path):
    from emdr2_amd.data import index_snapshot as snap
    n, dim, m = 5000, 64, 100
    path = str(tmp_path / "snap.flat")
    base = _base_meta(n, dim, True)
    with pytest.raises(FileNotFoundError):
        snap.read_delta_meta(path, base)
    rows, stamps, data, meta = _write_delta(path, n, dim, m, True, base)
    dpath, mpath = snap.delta_path(path), snap.delta_meta_path(path)
    good, good_meta = open(dpath, "rb").read(), open(mpath).read()

    def restore():
        open(dpath, "wb").write(good); open(mpath, "w").write(good_meta)
    # no meta: an incomplete delta
    os.remove(mpath)
    with pytest.raises(ValueError, match="incomplete"):
        snap.read_delta_meta(path, base)
    restore()
    # another format
    open(mpath, "w").write(json.dumps(dict(meta, format=2)))
    with pytest.raises(ValueError, match="format"):
        snap.read_delta_meta(path, base)
    restore()
    # wrong magic, wrong version, shorter than the header says
    open(dpath, "wb").write(b"EMDR2GEN" + good[8:])
    with pytest.raises(ValueError, match="not an index delta"):
        snap.read_delta_meta(path, base)
    open(dpath, "wb").write(good[:8] + b"\x02" + good[9:])
    with pytest.raises(ValueError, match="version 2"):
        snap.read_delta_meta(path, base)
    open(dpath, "wb").write(good[:-2])
    with pytest.raises(ValueError, match="shorter"):
        snap.read_delta_meta(path, base)
    open(dpath, "wb").write(good[:20])
    with pytest.raises(ValueError):
        snap.read_delta_meta(path, base)
    restore()
    # a base that is not this snapshot's: the rows' digest, the stamps' digest, stamps the base does not have
    for other in (dict(base, digest_xor="%016x" % 99), dict(base, stamps={"digest_sum": "%016x" % 13, "digest_xor": "%016x" % 15}),
                  _base_meta(n, dim, False)):
        with pytest.raises(ValueError, match="another base"):
            snap.read_delta_meta(path, other)
    # the row list is damaged
    flat = snap.DeltaFile(dpath, mode="r+"); flat.rows[m // 2] ^= 1; flat.flush(); del flat
    with pytest.raises(ValueError, match="checksum"):
        snap.read_delta_meta(path, base)
    restore()
    # a header that disagrees with the meta
    open(mpath, "w").write(json.dumps(dict(meta, m=m + 1)))
    with pytest.raises(ValueError, match="meta says"):
        snap.read_delta_meta(path, base)
    restore()
    assert snap.read_delta_meta(path, base) == meta
    snap.remove_delta(path)
    assert os.listdir(str(tmp_path)) == []
    snap.remove_delta(path)                                                                 # nothing there: nothing happens


# ---- the protocol, numpy shards --------------------------------------------------------------------------------------------------------------
class _NumpyShard(object):
    """Stands in for HipIndexShard: rows and, with `generations`, stamps on the host; digests and keys from the numpy restatements."""

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

    def set_stamps_at(self, local_rows, stamps):
        self.generation[np.asarray(local_rows)] = np.asarray(stamps).view(np.int32)

    def update_rows(self, local_row, rows, generation=None, newest_wins=False):
        self._rows[local_row:local_row + len(rows)] = rows
        if self.generation is not None:
            self.generation[local_row:local_row + len(rows)] = generation

    def update_rows_at(self, local_rows, rows, generation=None, newest_wins=False):
        local_rows = np.asarray(local_rows)
        mine = (local_rows >= 0) & (local_rows < self.n_rows)
        self._rows[local_rows[mine]] = np.asarray(rows)[mine]
        if self.generation is not None:
            self.generation[local_rows[mine]] = generation


def _index_class():
    from emdr2_amd.data import emdr2_index as ei

    class Index(ei.DistributedBruteForceIndex):
        def _make_shard(self, dim, n, base):
            return _NumpyShard(dim, n, base, self.generations)
    return Index


N, DIM = 1003, 64


def _data(n=N, dim=DIM):
    rng = np.random.default_rng(11)
    return (rng.permutation(n) + 1).astype(np.int32), rng.standard_normal((n, dim)).astype(np.float16)


def _changes(n, world, generation, seed):
    """The changes a world of `world` ranks makes after the base, as (global rows, fresh rows, stamp): per rank one range and one scattered
    list; rank r's range starts at its first row and its list holds its last row, so every rank's first and last row change."""
    from emdr2_amd.data.emdr2_index import shard_bounds
    rng = np.random.default_rng(seed)
    out = []
    for r, (lo, hi) in enumerate(shard_bounds(n, world)):
        span = np.arange(lo, lo + 20, dtype=np.int64)
        out.append((span, rng.standard_normal((20, DIM)).astype(np.float16), generation + r))
        ids = np.unique(np.concatenate([rng.choice(np.arange(lo + 20, hi), size=30, replace=False), [hi - 1]])).astype(np.int64)
        out.append((ids, rng.standard_normal((ids.size, DIM)).astype(np.float16), generation + 10 + r))
    return out


def _live(n, world, generations, changes):
    """what the index holds after `changes`: (rows, stamps)"""
    _, rows = _data(n)
    rows, stamps = rows.copy(), np.zeros(n, np.uint32)
    for ids, new, g in changes:
        rows[ids], stamps[ids] = new, g
    return rows, (stamps if generations else None)


def _apply(index, changes):
    lo, hi = index.local_rows()
    for ids, new, g in changes:
        mine = (ids >= lo) & (ids < hi)
        if mine.any():
            index.update_rows_at(ids[mine], new[mine], generation=g if index.generations else None)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, out_dir, action, generations):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from emdr2_amd.data import index_snapshot as snap
    path = os.path.join(out_dir, "snap.flat")
    verdict = "ok"
    index = _index_class()(embed_size=DIM, embed_data=None, use_gpu=True, generations=generations)
    if action.startswith("save"):
        ids, rows = _data()
        index.add_arrays(ids, rows)
        index.save_flat_file(path, meta={"iteration": 6, "mode": "rolling"}, track_deltas=True)
        assert index.delta_base is not None and index.delta_base["keys"].shape == (index.shard.n_rows,)
        _apply(index, _changes(N, 2, 7, 1))
        meta = index.save_delta(path, {"iteration": 9})
        assert meta["iteration"] == 9 and meta["world"] == world and meta == snap.read_delta_meta(path)
        if action == "save_twice":                          # cumulative: the second delta replaces the first, relative to the same base
            _apply(index, _changes(N, 2, 30, 2))
            again = index.save_delta(path, {"iteration": 12})
            assert again["base"] == meta["base"] and again["m"] > meta["m"]
        if action == "save_over":                           # rank 1 alone exceeds max_fraction: no rank writes, the stale delta is gone
            if rank == 1:
                lo, hi = index.local_rows()
                index.update_rows_at(np.arange(lo, hi, dtype=np.int64), np.ones((hi - lo, DIM), np.float16), generation=40 if generations else None)
            assert index.save_delta(path, {"iteration": 12}, max_fraction=0.5) is None
            assert not os.path.exists(snap.delta_path(path)) and not os.path.exists(snap.delta_meta_path(path))
    else:
        max_iteration = {"load": None, "load_at_9": 9, "load_at_8": 8}[action.split(":")[0]]
        changes = {"1": _changes(N, 2, 7, 1), "2": _changes(N, 2, 7, 1) + _changes(N, 2, 30, 2), "0": []}[action.split(":")[1]]
        meta = index.load_flat_snapshot(path, delta=True, max_iteration=max_iteration)
        rows, stamps = _live(N, 2, generations, changes)
        lo, hi = index.local_rows()
        assert np.array_equal(index.shard._rows.view(np.uint16), rows[lo:hi].view(np.uint16))
        if generations:
            assert np.array_equal(index.shard.generation[:hi - lo].view(np.uint32), stamps[lo:hi])
        if changes:
            assert index.delta_applied is not None and "delta_skipped" not in meta
            verdict = "applied %d" % index.delta_applied["iteration"]
        else:
            assert index.delta_applied is None
            verdict = "skipped: %s" % meta.get("delta_skipped")
        # the base's keys, not the live rows': this index's own next delta is relative to the same base
        _, base_rows = _data()
        base_stamps = np.zeros(N, np.uint32) if generations else None
        from emdr2_amd.data.emdr2_index import row_keys
        assert np.array_equal(index.delta_base["keys"], row_keys(base_rows[lo:hi], None if base_stamps is None else base_stamps[lo:hi], lo))
    with open(os.path.join(out_dir, "verdict%d.txt" % rank), "w") as fh:
        fh.write(verdict)
    dist.barrier()
    dist.destroy_process_group()


def _spawn(world, out_dir, action, generations):
    mp.spawn(_worker, args=(world, _free_port(), str(out_dir), action, generations), nprocs=world, join=True)
    return [open(os.path.join(str(out_dir), "verdict%d.txt" % r)).read() for r in range(world)]


@pytest.mark.parametrize("generations", [False, True])
def test_gloo_world_2_writes_a_delta_that_worlds_1_and_3_load(tmp_path, generations):
    from emdr2_amd.data import index_snapshot as snap
    from emdr2_amd.data.emdr2_index import digest_rows, digest_stamps
    path = str(tmp_path / "snap.flat")
    assert _spawn(2, tmp_path, "save", generations) == ["ok"] * 2
    names = ["snap.flat", "snap.flat.delta", "snap.flat.delta.meta"] + (["snap.flat.gen"] if generations else []) + ["snap.flat.meta"]
    assert sorted(n for n in os.listdir(str(tmp_path)) if n.startswith("snap")) == names   # no part file is left
    changes = _changes(N, 2, 7, 1)
    rows, stamps = _live(N, 2, generations, changes)
    changed = np.unique(np.concatenate([c[0] for c in changes]))
    assert {0, 501, 502, N - 1} <= set(changed.tolist())                                   # each rank's first and last row
    flat, meta = snap.DeltaFile(snap.delta_path(path)), snap.read_delta_meta(path)
    assert np.array_equal(flat.rows, changed) and np.array_equal(flat.data.view(np.uint16), rows[changed].view(np.uint16))
    assert flat.stamped == generations and (not generations or np.array_equal(flat.stamps, stamps[changed]))
    s, x = digest_rows(rows)
    want = {"digest_sum": "%016x" % s, "digest_xor": "%016x" % x}
    if generations:
        want["stamps"] = dict(zip(("digest_sum", "digest_xor"), ("%016x" % v for v in digest_stamps(stamps))))
    assert meta["result"] == want and meta["base"] == snap.base_of(snap.read_snapshot_meta(path))
    assert (meta["format"], meta["m"], meta["n"], meta["dim"], meta["world"], meta["iteration"]) == (1, changed.size, N, DIM, 2, 9)
    for world in (1, 3):
        assert _spawn(world, tmp_path, "load:1", generations) == ["applied 9"] * world
    assert _spawn(3, tmp_path, "load_at_9:1", generations) == ["applied 9"] * 3
    # a delta newer than the checkpoint is skipped, the base alone is loaded
    verdicts = _spawn(2, tmp_path, "load_at_8:0", generations)
    assert verdicts == ["skipped: the delta is of iteration 9, beyond 8"] * 2
    # a result digest that the loaded rows do not have: every rank refuses, naming both
    bad = dict(meta, result=dict(meta["result"], digest_xor="%016x" % 5))
    open(snap.delta_meta_path(path), "w").write(json.dumps(bad))
    index = _index_class()(embed_size=DIM, embed_data=None, use_gpu=True, generations=generations)
    with pytest.raises(ValueError, match="%016x %016x in HBM, %016x %016x in the delta's meta" % (s, x, s, 5)):
        index.load_flat_snapshot(path, delta=True)
    # a delta of another base is skipped with the reason, not raised
    open(snap.delta_meta_path(path), "w").write(json.dumps(dict(meta, base=dict(meta["base"], digest_sum="%016x" % 1))))
    out = index.load_flat_snapshot(path, delta=True)
    assert index.delta_applied is None and "another base" in out["delta_skipped"]
    # without delta=True nothing of this is looked at
    assert "delta_skipped" not in index.load_flat_snapshot(path) and index.delta_applied is None


def test_gloo_a_second_delta_replaces_the_first(tmp_path):
    assert _spawn(2, tmp_path, "save_twice", True) == ["ok"] * 2
    assert _spawn(3, tmp_path, "load:2", True) == ["applied 12"] * 3


def test_gloo_max_fraction_exceeded_on_one_rank_writes_nothing_anywhere(tmp_path):
    assert _spawn(2, tmp_path, "save_over", True) == ["ok"] * 2
    assert sorted(os.listdir(str(tmp_path))) == ["snap.flat", "snap.flat.gen", "snap.flat.meta", "verdict0.txt", "verdict1.txt"]


def _single(generations=True, track=True, tmp_path=None):
    ids, rows = _data()
    index = _index_class()(embed_size=DIM, embed_data=None, use_gpu=True, generations=generations)
    index.add_arrays(ids, rows)
    path = str(tmp_path / "snap.flat")
    index.save_flat_file(path, meta={"iteration": 6}, track_deltas=track)
    return index, path


def test_a_failed_writer_removes_its_part_file(tmp_path, monkeypatch):
    from emdr2_amd.data import index_snapshot as snap
    index, path = _single(tmp_path=tmp_path)
    _apply(index, _changes(N, 1, 7, 1))
    assert index.save_delta(path, {"iteration": 7}) is not None
    before = open(snap.delta_path(path), "rb").read()

    def fail(*a, **k):
        raise PermissionError(13, "Permission denied")
    monkeypatch.setattr(snap, "_write_slice", fail)
    _apply(index, _changes(N, 1, 20, 2))
    with pytest.raises(PermissionError):
        index.save_delta(path, {"iteration": 8})
    assert sorted(os.listdir(str(tmp_path))) == ["snap.flat", "snap.flat.delta", "snap.flat.delta.meta", "snap.flat.gen", "snap.flat.meta"]
    assert open(snap.delta_path(path), "rb").read() == before and snap.read_delta_meta(path)["iteration"] == 7   # the old delta stays valid


def test_save_delta_without_a_base_and_the_untracked_save(tmp_path):
    """`save_flat_file` without `track_deltas` leaves exactly the files it left before and no `delta_base`; `save_delta` then writes
    nothing, removes a stale delta and says why.  A new base removes the delta of the one it replaces."""
    from emdr2_amd.data import index_snapshot as snap
    index, path = _single(track=False, tmp_path=tmp_path)
    assert index.delta_base is None and sorted(os.listdir(str(tmp_path))) == ["snap.flat", "snap.flat.gen", "snap.flat.meta"]
    open(snap.delta_path(path), "wb").write(b"stale"); open(snap.delta_meta_path(path), "w").write("{}")
    said = []
    assert index.save_delta(path, {"iteration": 7}, log=said.append) is None
    assert sorted(os.listdir(str(tmp_path))) == ["snap.flat", "snap.flat.gen", "snap.flat.meta"]
    assert len(said) == 1 and "skipped" in said[0] and "no base" in said[0]
    # tracked: an empty delta (nothing changed) is a delta; the next base removes it; keys of another path are no base here
    index.save_flat_file(path, meta={"iteration": 8}, track_deltas=True)
    meta = index.save_delta(path, {"iteration": 9}, log=said.append)
    assert meta["m"] == 0 and meta["result"] == {k: v for k, v in snap.read_snapshot_meta(path).items() if k in ("digest_sum", "digest_xor", "stamps")}
    assert "0 of %d rows" % N in said[-1]
    assert index.save_delta(str(tmp_path / "elsewhere.flat"), {"iteration": 9}) is None
    index.save_flat_file(path, meta={"iteration": 10}, track_deltas=True)
    assert sorted(os.listdir(str(tmp_path))) == ["snap.flat", "snap.flat.gen", "snap.flat.meta"]


def test_the_paced_writer_keeps_the_keys_of_the_bits_in_the_file(tmp_path):
    """Chunks of 100 rows with updates between the pumps, ahead of and behind the cursor: base + delta is the live index."""
    from emdr2_amd.data import index_snapshot as snap
    ids, rows = _data()
    Index = _index_class()
    index = Index(embed_size=DIM, embed_data=None, use_gpu=True, generations=True)
    index.add_arrays(ids, rows)
    path = str(tmp_path / "snap.flat")
    writer = snap.IndexSnapshotWriter(index, chunk_rows=100, track_deltas=True)
    writer.begin(path, {"iteration": 3})
    rng = np.random.default_rng(5)
    g = 10
    while not writer.pump():
        g += 1
        hit = rng.choice(N, size=40, replace=False).astype(np.int64)
        index.update_rows_at(hit, rng.standard_normal((40, DIM)).astype(np.float16), generation=g)
        assert index.delta_base is None                                                    # nothing is published yet
    writer.finish()
    meta = index.save_delta(path, {"iteration": 30})
    assert 0 < meta["m"] < N
    fresh = Index(embed_size=DIM, embed_data=None, use_gpu=True, generations=True)
    fresh.load_flat_snapshot(path, delta=True)
    assert fresh.delta_applied == meta
    assert np.array_equal(fresh.shard._rows.view(np.uint16), index.shard._rows.view(np.uint16))
    assert np.array_equal(fresh.shard.generation, index.shard.generation)


# ---- the C entry points refuse bad arguments before any launch -----------------------------------------------------------------------------
def _lib():
    import __graft_entry__ as g
    from emdr2_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        g.build()
    return _native.lib()


def test_row_keys_entry_point_validates_arguments_without_a_gpu():
    fn = _lib().emdr2_mips_row_keys
    one, off4, off2 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4), ctypes.c_void_p(4096 + 2)
    assert fn(None, 1000, 64, 0, 10, 0, None, one, None) == -1                             # null image
    assert fn(one, 1000, 64, 0, 10, 0, None, None, None) == -1                             # null keys
    assert fn(one, 1000, 64, 0, 10, 0, None, off4, None) == -1                             # keys are 8-byte words
    assert fn(one, 1000, 64, 0, 10, 0, off2, one, None) == -1                              # stamps are 4-byte words
    assert fn(one, 1000, 32, 0, 10, 0, None, one, None) == -1 and fn(one, 1000, 80, 0, 10, 0, None, one, None) == -1      # the layout's envelope
    assert fn(one, 1000, 64, -1, 10, 0, None, one, None) == -1 and fn(one, 1000, 64, 0, -1, 0, None, one, None) == -1
    assert fn(one, 1000, 64, 991, 10, 0, None, one, None) == -1 and fn(one, 1000, 64, 0, 10, -1, None, one, None) == -1
    assert fn(one, 2 ** 31, 64, 0, 10, 0, None, one, None) == -1
    assert fn(one, 1000, 64, 1000, 0, 0, None, one, None) == 0 and fn(one, 1000, 64, 0, 0, 0, off4, one, None) == 0      # an empty range: no launch


def test_changed_rows_entry_points_validate_arguments_without_a_gpu():
    lib = _lib()
    size = ctypes.c_size_t()
    ws_bytes = lib.emdr2_mips_changed_rows_workspace_bytes
    assert ws_bytes(1000, None) == -1 and ws_bytes(-1, ctypes.byref(size)) == -1 and ws_bytes(2 ** 31, ctypes.byref(size)) == -1
    assert ws_bytes(0, ctypes.byref(size)) == 0 and size.value == 512 * 40                 # the per-slab words alone
    assert ws_bytes(1000, ctypes.byref(size)) == 0
    need = size.value
    assert need == 8 * (16 + 32) + 512 * 40 + 32                                           # 8 stripes: mask, digest words; slabs; counts padded to 16
    fn = lib.emdr2_mips_changed_rows
    one, off8, off4, off2 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8), ctypes.c_void_p(4096 + 4), ctypes.c_void_p(4096 + 2)

    def call(tiled=one, n=1000, dim=64, base=0, gen=None, keys=one, cap=10, rows=one, info=one, ws=one, nbytes=need):
        return fn(tiled, n, dim, base, gen, keys, cap, rows, info, ws, nbytes, None)
    assert call(tiled=None) == -1 and call(keys=None) == -1 and call(rows=None) == -1 and call(info=None) == -1 and call(ws=None) == -1
    assert call(keys=off4) == -1 and call(rows=off4) == -1 and call(info=off4) == -1 and call(ws=off8) == -1 and call(gen=off2) == -1
    assert call(dim=32) == -1 and call(dim=80) == -1 and call(n=-1) == -1 and call(n=2 ** 31, cap=0) == -1 and call(base=-1) == -1
    assert call(cap=-1) == -1 and call(cap=1001) == -1
    assert call(nbytes=need - 1) == -2 and call(nbytes=0) == -2                            # the workspace is too small
