"""Snapshots of the evidence index that lives in HBM: one `FlatEmbeddingFile` plus a JSON meta file, written by all ranks together.

The reference's indexer group rewrites `--embedding-path` at every refresh, so a resumed or finished run has the index that matches its
checkpoint.  Here the refreshed index exists only in the trainers' HBM (tasks/openqa/e2eqa/async_indexer.py); this module is its way
out.  Protocol (`IndexSnapshotWriter`; `DistributedBruteForceIndex.save_flat_file` is `begin` + `finish`):

  1. rank 0 creates `<path>.part.<host>.<uuid>` at full size; barrier
  2. every rank exports its shard chunk by chunk (emdr2_mips_export_rows -> pinned buffer -> its slice of the file) and folds the DEVICE
     digest of exactly what it exported (emdr2_mips_digest_rows)
  3. every rank's slice is on disk; the per-rank digests are all-gathered as int64 bit patterns and combined on the host mod 2^64
  4. rank 0 removes an old `<path>.meta`, renames the data file onto `<path>`, then writes `<path>.meta` (tmp + rename)

A data file without a meta is therefore an incomplete snapshot and is refused (`read_snapshot_meta`).  Any world size reads a snapshot
written by any other: the file is the whole index in global row order, and the digest does not depend on how the rows were cut.

Generation stamps.  A snapshot of an index whose shards keep stamps (`shard.generation`) also stores every row's stamp, in the sidecar
`<path>.gen` (`StampFile`):

    8-byte magic "EMDR2GEN" | u32 version = 1 | u32 0 | u64 n | n little-endian uint32 stamps in GLOBAL row order

In step 1 rank 0 creates `<tmp>.gen` at full size as well; in step 2 a chunk's stamps are taken on the same stream, between the same two
neighbours, as its rows, and their device digest (emdr2_mips_digest_stamps) is folded into a second accumulator; step 3 gathers both
digests in the one all-gather; step 4 becomes: remove the old meta, rename the sidecar, rename the data file, write the meta, which gains
the one key `"stamps": {"digest_sum": hex, "digest_xor": hex}`.  A meta that names stamps without a matching sidecar is an incomplete
snapshot.  A snapshot of an index without stamps has neither the key nor a sidecar (a stale one is removed), and its meta and data file
are what they always were; `"format"` stays 1 either way.

Incremental snapshots.  A writer with `track_deltas` also keeps, for every row it exports, the row's KEY (emdr2_mips_row_keys:
the row hash of the digest, plus the stamp hash on a stamped index), taken at the same stream point as the export; after the publish the
index holds them as `index.delta_base`.  `save_delta` then finds the rows whose key differs (emdr2_mips_changed_rows) and writes only those
next to the base, always relative to the published base -- one file, overwritten atomically, no chain:

    `<path>.delta`       8-byte magic "EMDR2DLT" | u32 version = 1 | u32 flags (bit 0: stamps) | u64 m | u32 dim | u32 0, then, each section
                         16-byte aligned: int64 global rows [m] ascending | uint32 stamps [m] if flagged | fp16 rows [m, dim]
    `<path>.delta.meta`  JSON: format, m, n, dim, world, iteration, `base` (the base meta's digests), `result` (the digests of base + delta,
                         from the device at the stream point of the detection pass), rows_crc32, and the caller's keys

The ranks fill disjoint slices of `<path>.delta.part.<host>.<uuid>`; rank 0 removes the old delta meta, renames the data file and writes the
meta last.  A delta without a meta, or whose `base` is not the base snapshot's, is not a delta of this base (`read_delta_meta`).
"""
import json
import os
import queue
import socket
import struct
import threading
import uuid
import zlib

import numpy as np
import torch

SNAPSHOT_NAME = 'evidence_index.flat'   # the one snapshot file of a training run, under --save (--save-index-snapshot)
SNAPSHOT_FORMAT = 1
SNAPSHOT_ROWS = 1 << 18             # rows per chunk of a synchronous save (at most emdr2_index._UPLOAD_ROWS; 384 MiB of pinned memory at D = 768)
_MASK = 2 ** 64 - 1


def _to_i64(u):
    return u - 2 ** 64 if u >= 2 ** 63 else u


def _unique():
    return "%s.%s" % (socket.gethostname(), uuid.uuid4().hex)


def meta_path(path):
    return path + '.meta'


def stamps_path(path):
    return path + '.gen'


STAMPS_MAGIC = b'EMDR2GEN'
_STAMPS_HEADER = 24


class StampFile(object):
    """The sidecar of a snapshot with generation stamps: header (module docstring) + `stamps`, uint32 [n] in global row order, memory-mapped.
    ValueError for another magic or version, or a file shorter than its header says."""

    def __init__(self, path, mode='r'):
        self.path = path
        with open(path, 'rb') as f:
            head = f.read(_STAMPS_HEADER)
        if len(head) < _STAMPS_HEADER or head[:8] != STAMPS_MAGIC:
            raise ValueError("not a generation stamp file: %s" % path)
        version, _, self.n = struct.unpack('<IIQ', head[8:])
        if version != 1:
            raise ValueError("unsupported generation stamp file version %d" % version)
        if os.path.getsize(path) < _STAMPS_HEADER + 4 * self.n:
            raise ValueError("generation stamp file is shorter than its header says: %s" % path)
        # (numpy cannot map zero bytes)
        self.stamps = np.memmap(path, dtype='<u4', mode=mode, offset=_STAMPS_HEADER, shape=(self.n,)) if self.n else np.empty((0,), '<u4')

    @classmethod
    def create(cls, path, n):
        """Header + a file of full size (zeros), opened writable: several processes fill disjoint slices through maps of their own."""
        with open(path, 'wb') as f:
            f.write(STAMPS_MAGIC)
            f.write(struct.pack('<IIQ', 1, 0, int(n)))
            f.truncate(_STAMPS_HEADER + 4 * int(n))
        return cls(path, mode='r+')

    @staticmethod
    def write(path, stamps):
        stamps = np.ascontiguousarray(stamps)
        if stamps.dtype not in (np.dtype(np.uint32), np.dtype(np.int32)) or stamps.ndim != 1:
            raise ValueError("stamps must be uint32 or int32 [n]")
        with open(path, 'wb') as f:
            f.write(STAMPS_MAGIC)
            f.write(struct.pack('<IIQ', 1, 0, stamps.shape[0]))
            f.write(stamps.view(np.uint32).astype('<u4').tobytes())

    def flush(self):
        if isinstance(self.stamps, np.memmap):
            self.stamps.flush()


def ids_crc32(ids):
    crc = 0
    for lo in range(0, ids.shape[0], 1 << 22):
        crc = zlib.crc32(np.ascontiguousarray(ids[lo:lo + (1 << 22)], dtype=np.int32).tobytes(), crc)
    return crc & 0xffffffff


def delta_path(path):
    return path + '.delta'


def delta_meta_path(path):
    return path + '.delta.meta'


DELTA_MAGIC = b'EMDR2DLT'
DELTA_FORMAT = 1
_DELTA_HEADER = 32
DELTA_ROWS = 1 << 16                # rows per chunk of a delta's copies to and from the host


def _align16(x):
    return (x + 15) // 16 * 16


class DeltaFile(object):
    """`<path>.delta` (module docstring), memory-mapped: `rows` int64 [m] global rows, `stamps` uint32 [m] or None, `data` fp16 [m, dim].
    ValueError for another magic or version, or a file shorter than its header says."""

    def __init__(self, path, mode='r'):
        self.path = path
        with open(path, 'rb') as f:
            head = f.read(_DELTA_HEADER)
        if len(head) < _DELTA_HEADER or head[:8] != DELTA_MAGIC:
            raise ValueError("not an index delta file: %s" % path)
        version, flags, self.m, self.dim, _ = struct.unpack('<IIQII', head[8:])
        if version != 1:
            raise ValueError("unsupported index delta file version %d" % version)
        self.stamped = bool(flags & 1)
        rows_at, stamps_at, data_at, size = self.layout(self.m, self.dim, self.stamped)
        if os.path.getsize(path) < size:
            raise ValueError("index delta file is shorter than its header says: %s" % path)
        m, dim = self.m, self.dim
        # (numpy cannot map zero bytes)
        self.rows = np.memmap(path, dtype='<i8', mode=mode, offset=rows_at, shape=(m,)) if m else np.empty((0,), '<i8')
        self.stamps = (np.memmap(path, dtype='<u4', mode=mode, offset=stamps_at, shape=(m,)) if m else np.empty((0,), '<u4')) if self.stamped else None
        self.data = np.memmap(path, dtype='<f2', mode=mode, offset=data_at, shape=(m, dim)) if m else np.empty((0, dim), '<f2')

    @staticmethod
    def layout(m, dim, stamped):
        """-> the offsets of the three sections (the stamps' is the data's when there are none) and the file's size"""
        rows_at = _DELTA_HEADER
        stamps_at = _align16(rows_at + 8 * m)
        data_at = _align16(stamps_at + 4 * m) if stamped else stamps_at
        return rows_at, stamps_at, data_at, data_at + 2 * m * dim

    @classmethod
    def create(cls, path, m, dim, stamped):
        """Header + a file of full size (zeros), opened writable: several processes fill disjoint slices through maps of their own."""
        with open(path, 'wb') as f:
            f.write(DELTA_MAGIC)
            f.write(struct.pack('<IIQII', 1, 1 if stamped else 0, int(m), int(dim), 0))
            f.truncate(cls.layout(int(m), int(dim), stamped)[3])
        return cls(path, mode='r+')

    def flush(self):
        for part in (self.rows, self.stamps, self.data):
            if isinstance(part, np.memmap):
                part.flush()


def rows_crc32(rows):
    crc = 0
    for lo in range(0, rows.shape[0], 1 << 21):
        crc = zlib.crc32(np.ascontiguousarray(rows[lo:lo + (1 << 21)], dtype='<i8').tobytes(), crc)
    return crc & 0xffffffff


def base_of(meta):
    """What a delta's meta records of its base: the base meta's digests."""
    base = {"digest_sum": meta["digest_sum"], "digest_xor": meta["digest_xor"]}
    if meta.get("stamps") is not None:
        base["stamps"] = {"digest_sum": meta["stamps"]["digest_sum"], "digest_xor": meta["stamps"]["digest_xor"]}
    return base


def read_delta_meta(path, base_meta=None):
    """The meta of the delta next to the snapshot at `path`, validated against the delta file and the base snapshot's meta (read from
    `path` when not given) -> dict.  FileNotFoundError when there is no delta file; ValueError, saying which, for a delta without a meta,
    another format, a `base` that is not this snapshot's, a header or a row list that disagrees with the meta."""
    if not os.path.exists(delta_path(path)):
        raise FileNotFoundError("no index delta at %s" % delta_path(path))
    if not os.path.exists(delta_meta_path(path)):
        raise ValueError("%s has no %s: an incomplete delta" % (delta_path(path), os.path.basename(delta_meta_path(path))))
    with open(delta_meta_path(path)) as fh:
        meta = json.load(fh)
    if meta.get("format") != DELTA_FORMAT:
        raise ValueError("unsupported index delta format %r" % (meta.get("format"),))
    if base_meta is None:
        base_meta = read_snapshot_meta(path)
    if meta.get("base") != base_of(base_meta):
        raise ValueError("index delta %s is relative to another base (%r), not to this snapshot (%r)"
                         % (delta_path(path), meta.get("base"), base_of(base_meta)))
    flat = DeltaFile(delta_path(path))
    if (meta.get("m"), meta.get("dim"), meta.get("n")) != (flat.m, flat.dim, base_meta["n"]) or flat.dim != base_meta["dim"]:
        raise ValueError("delta meta says %r rows x %r of %r, the file %d x %d, the base %d x %d"
                         % (meta.get("m"), meta.get("dim"), meta.get("n"), flat.m, flat.dim, base_meta["n"], base_meta["dim"]))
    for key in ("digest_sum", "digest_xor"):
        int(meta["result"][key], 16)
    if meta["result"].get("stamps") is not None:
        for key in ("digest_sum", "digest_xor"):
            int(meta["result"]["stamps"][key], 16)
    int(meta["iteration"])
    rows = flat.rows
    if rows_crc32(rows) != meta.get("rows_crc32"):
        raise ValueError("index delta %s: the row list does not match the meta's checksum" % delta_path(path))
    if flat.m and (int(rows[0]) < 0 or int(rows[-1]) >= base_meta["n"] or (flat.m > 1 and not bool(np.all(rows[1:] > rows[:-1])))):
        raise ValueError("index delta %s: the row list is not ascending inside [0, %d)" % (delta_path(path), base_meta["n"]))
    return meta


def remove_delta(path):
    """Remove the delta next to the snapshot at `path`, meta first (a delta without a meta is no delta)."""
    for part in (delta_meta_path(path), delta_path(path)):
        try:
            os.remove(part)
        except FileNotFoundError:
            pass


def read_snapshot_meta(path):
    """The meta of the snapshot at `path`, validated against the data file's header -> dict.  Raises ValueError for a data file without
    a meta (an incomplete snapshot), an unknown format, or a header that disagrees; FileNotFoundError when there is no data file.  A meta
    that names `stamps` needs its sidecar: a missing one, one whose header holds another n, or one shorter than its header says is an
    incomplete snapshot too."""
    from emdr2_amd.data.emdr2_index import FlatEmbeddingFile
    if not os.path.exists(path):
        raise FileNotFoundError("no index snapshot at %s" % path)
    if not os.path.exists(meta_path(path)):
        raise ValueError("%s has no %s: an incomplete snapshot" % (path, os.path.basename(meta_path(path))))
    with open(meta_path(path)) as fh:
        meta = json.load(fh)
    if meta.get("format") != SNAPSHOT_FORMAT:
        raise ValueError("unsupported index snapshot format %r" % (meta.get("format"),))
    flat = FlatEmbeddingFile(path)
    if (meta.get("n"), meta.get("dim")) != (flat.n, flat.dim):
        raise ValueError("snapshot meta says %r x %r, the file %d x %d" % (meta.get("n"), meta.get("dim"), flat.n, flat.dim))
    for key in ("digest_sum", "digest_xor"):
        int(meta[key], 16)
    if meta.get("stamps") is not None:
        for key in ("digest_sum", "digest_xor"):
            int(meta["stamps"][key], 16)
        if not os.path.exists(stamps_path(path)):
            raise ValueError("%s names stamps and has no %s: an incomplete snapshot" % (path, os.path.basename(stamps_path(path))))
        n = StampFile(stamps_path(path)).n
        if n != flat.n:
            raise ValueError("snapshot stamp file holds %d stamps, the data file %d rows" % (n, flat.n))
    return meta


class _Collective(object):
    """The three collectives of a snapshot over the index's process group; without torch.distributed: one rank."""

    def __init__(self, index):
        self.group = index.process_group
        self.rank, self.world = index._world()
        self.on = self.world > 1 or (torch.distributed.is_available() and torch.distributed.is_initialized())
        self.device = "cpu"
        if self.on and torch.distributed.get_backend(self.group) == "nccl":
            self.device = torch.device("cuda", torch.cuda.current_device())

    def barrier(self):
        if self.on:
            torch.distributed.barrier(self.group)

    def share(self, value):
        """rank 0's picklable `value` on every rank"""
        if not self.on:
            return value
        box = [value if self.rank == 0 else None]
        src = torch.distributed.get_global_rank(self.group, 0) if self.group is not None else 0
        torch.distributed.broadcast_object_list(box, src=src, group=self.group, device=torch.device(self.device))
        return box[0]

    def minimum(self, value):
        if not self.on:
            return value
        t = torch.tensor([value], dtype=torch.int32, device=self.device)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MIN, group=self.group)
        return int(t.item())

    def gather_words(self, words):
        """This rank's list of ints below 2^64 -> every rank's list, in rank order (one all-gather of int64 bit patterns)."""
        if not self.on:
            return [[w & _MASK for w in words]]
        mine = torch.tensor([_to_i64(w & _MASK) for w in words], dtype=torch.int64, device=self.device)
        out = torch.empty((self.world * mine.numel(),), dtype=torch.int64, device=self.device)
        torch.distributed.all_gather_into_tensor(out, mine, group=self.group)
        flat, k = out.tolist(), mine.numel()
        return [[w & _MASK for w in flat[k * r:k * (r + 1)]] for r in range(self.world)]

    def gather_digests(self, pair, *more):
        """This rank's (sum, xor) -> the digest over all ranks: the pairs travel as int64 bit patterns in one all-gather and are combined
        on the host mod 2^64 (an all-reduce would add int64s: signed overflow, and no XOR over every transport).  With `more` pairs (the
        stamps' next to the rows'): all of them in the SAME all-gather -> the list of their digests."""
        from emdr2_amd.data.emdr2_index import combine_digests
        pairs = (pair,) + more
        if not self.on:
            flat, world = [w for p in pairs for w in p], 1
        else:
            mine = torch.tensor([_to_i64(w) for p in pairs for w in p], dtype=torch.int64, device=self.device)
            out = torch.empty((self.world * mine.numel(),), dtype=torch.int64, device=self.device)
            torch.distributed.all_gather_into_tensor(out, mine, group=self.group)
            flat, world = out.tolist(), self.world
        k = 2 * len(pairs)
        digests = [combine_digests([(flat[k * r + 2 * i] & _MASK, flat[k * r + 2 * i + 1] & _MASK) for r in range(world)]) for i in range(len(pairs))]
        return digests if more else digests[0]


def index_digest(index):
    """Device digest of the whole index, combined over the ranks that share it (collective; one readback per rank)."""
    return _Collective(index).gather_digests(index.shard.digest())


def index_stamp_digest(index):
    """Device digest of the generation stamps of the whole index, combined over the ranks that share it (collective; one readback per rank)."""
    return _Collective(index).gather_digests(index.shard.digest_stamps())


class IndexSnapshotWriter(object):
    """Writes the index's live image to one flat file, a chunk per `pump()`, without ever blocking the step.

        writer.begin(path, meta)        collective, at a rank-uniform point (a swap boundary)
        writer.pump()                   every step boundary, after the refresher's `maybe_swap`
        writer.maybe_finalize(it)       every step boundary; collective only when it % 10 == 0
        writer.finish()                 blocking: drain, join, re-raise, finalise

    `pump()` exports the next chunk ON THE CURRENT STREAM (after a rolling refresher's `update_rows` of this boundary, before the next
    step's searches: a row is exported whole, old or new, never torn) and folds its digest on the same stream, so the digest in the meta is
    that of exactly the exported bits.  The device-to-host copy into one of two pinned buffers runs on a side stream behind an event; ONE
    background thread waits for that event (its only GPU call) and writes the slice through the file's memory map.  With no free buffer
    `pump()` does nothing this step.  In swap mode the live image does not change between swaps, so the file equals the committed image;
    in rolling mode it is a mix of generations, as the live index is.

    A shard with generation stamps: the chunk's stamps are copied and digested on the current stream right next to its rows, with no
    writer between the four calls -- a stamped update enqueued before the pump is in both the row and its stamp, one enqueued after it in
    neither.  `shard.generation` is read at every pump (`commit_refresh` swaps the array).  The stamps ride the same side stream, the same
    event and the same buffer cycle to the host, and the background thread writes them to the sidecar (module docstring).

    `track_deltas`: the chunk's row keys (`shard.row_keys`) are taken at that stream point as well, into a key array of this snapshot's
    own -- the keys of exactly the bits in the file, also for a rolling, paced snapshot.  After the publish the index holds them as
    `index.delta_base`; until then the old base, its keys and its delta stay valid."""

    def __init__(self, index, chunk_rows=None, log=None, track_deltas=False):
        self.index = index
        self.chunk_rows = chunk_rows
        self.track_deltas = bool(track_deltas)                     # keep every exported row's key: the base of later `save_delta`s
        self.log = log or (lambda msg: None)
        self.active = False

    @staticmethod
    def paced_chunk_rows(n_rows, index_reload_interval):
        """Default pace in training: the shard is covered in half a reload interval of pumps."""
        pumps = max(1, int(index_reload_interval) // 2)
        return max(1, min(SNAPSHOT_ROWS, (n_rows + pumps - 1) // pumps))

    # -- collective -------------------------------------------------------------------------------------------------------------------
    def begin(self, path, meta=None, chunk_rows=None):
        from emdr2_amd.data.emdr2_index import FlatEmbeddingFile
        if self.active:
            raise RuntimeError("a snapshot is already being written (%s)" % self.path)
        index, shard = self.index, self.index.shard
        if shard is None:
            raise RuntimeError("MIPS Index is not initialized")
        self.coll = _Collective(index)
        self.path, self.meta = path, dict(meta or {})
        self._tmp = self.coll.share(path + '.part.' + _unique())
        self._stamped = getattr(shard, "generation", None) is not None      # (every rank's shard keeps stamps, or none does)
        err = None
        if self.coll.rank == 0:
            try:
                FlatEmbeddingFile.create(self._tmp, index.num_rows, index.embed_size)
                if self._stamped:
                    StampFile.create(stamps_path(self._tmp), index.num_rows)
            except Exception as exc:                               # the peers are waiting at the barrier: meet them first, then raise
                err = exc
                self._remove_parts()
        if self.coll.minimum(0 if err is not None else 1) == 0:    # (also the barrier "the files exist")
            raise err if err is not None else RuntimeError("rank 0 could not create %s" % self._tmp)
        self._file = FlatEmbeddingFile(self._tmp, mode='r+')
        self._gen_file = StampFile(stamps_path(self._tmp), mode='r+') if self._stamped else None
        self._n, self._cursor = shard.n_rows, 0
        self._chunk = max(1, int(chunk_rows or self.chunk_rows or SNAPSHOT_ROWS))
        self._chunk = min(self._chunk, max(self._n, 1))
        self._cuda = bool(getattr(shard, "tiled", None) is not None and shard.tiled.is_cuda)
        self._host_digest = self._host_stamp_digest = (0, 0)
        if self._cuda:
            self._acc = torch.zeros(4, dtype=torch.int64, device=shard.device)      # the rows' (sum, xor), then the stamps'
            self._dev = [torch.empty((self._chunk, shard.dim), dtype=torch.float16, device=shard.device) for _ in range(2)]
            self._pinned = [torch.empty((self._chunk, shard.dim), dtype=torch.float16).pin_memory() for _ in range(2)]
            if self._stamped:
                self._gen_dev = [torch.empty(self._chunk, dtype=torch.int32, device=shard.device) for _ in range(2)]
                self._gen_pinned = [torch.empty(self._chunk, dtype=torch.int32).pin_memory() for _ in range(2)]
            self._side = torch.cuda.Stream(device=shard.device)
        self._keys = None
        if self.track_deltas:
            self._keys = (torch.empty(self._n, dtype=torch.int64, device=shard.device) if self._cuda else np.empty(self._n, dtype=np.uint64))
        ids = shard.ids if shard.ids is not None else np.arange(shard.row_base, shard.row_base + self._n, dtype=np.int32)
        ids = ids.cpu().numpy() if torch.is_tensor(ids) else np.asarray(ids, dtype=np.int32)
        self._free = queue.Queue()
        for b in range(2):
            self._free.put(b)
        self._work = queue.Queue()
        self._error = None
        self._written = threading.Event()
        self._thread = threading.Thread(target=self._write_loop, name="index-snapshot", daemon=True)
        self._thread.start()
        self._work.put(("ids", ids))
        if self._n == 0:
            self._work.put(None)
        self.active = True

    def _write_loop(self):
        """The background thread: wait for a chunk's copy event, write the slice.  After an error it keeps handing buffers back (so a
        blocking `finish()` ends) and writes nothing more."""
        base = self.index.shard.row_base
        while True:
            item = self._work.get()
            try:
                if item is None:
                    if self._error is None:
                        self._file.flush()
                        if self._gen_file is not None:
                            self._gen_file.flush()
                    return
                if self._error is not None:
                    continue
                if item[0] == "ids":
                    self._file.ids[base:base + self._n] = item[1]
                else:
                    _, buf, lo, m, event, host, stamps = item
                    if event is not None:
                        event.synchronize()
                        host = self._pinned[buf][:m].numpy()
                        stamps = self._gen_pinned[buf][:m].numpy().view(np.uint32) if self._stamped else None
                    self._file.rows[base + lo:base + lo + m] = host
                    if stamps is not None:
                        self._gen_file.stamps[base + lo:base + lo + m] = stamps
            except BaseException as exc:                           # surfaces from finish() / maybe_finalize()
                self._error = exc
            finally:
                if item is None:
                    self._written.set()
                elif item[0] == "rows" and item[1] is not None:
                    self._free.put(item[1])

    def _pump_one(self, block):
        shard = self.index.shard
        lo, m = self._cursor, min(self._chunk, self._n - self._cursor)
        if not self._cuda:
            # a host stand-in for the shard (CPU tests): its rows are already on the host, nothing to overlap
            rows = shard.export_rows(lo, m)
            from emdr2_amd.data.emdr2_index import combine_digests, digest_stamps
            self._host_digest = combine_digests([self._host_digest, shard.digest(lo, m)])
            stamps = None
            if self._stamped:
                stamps = np.array(np.asarray(shard.generation)[lo:lo + m], copy=True).view(np.uint32)
                self._host_stamp_digest = combine_digests([self._host_stamp_digest, digest_stamps(stamps, shard.row_base + lo)])
            if self._keys is not None:
                self._keys[lo:lo + m] = host_shard_keys(shard, lo, m)
            self._work.put(("rows", None, lo, m, None, np.array(rows, dtype=np.float16, copy=True), stamps))
        else:
            try:
                buf = self._free.get(block=block)
            except queue.Empty:
                return False
            cur = torch.cuda.current_stream(shard.device)
            shard.export_rows(lo, m, out=self._dev[buf])
            shard.digest_into(self._acc[:2], lo, m)
            if self._stamped:                                      # (the same stream point: no writer is enqueued between these four)
                shard.export_stamps(lo, m, out=self._gen_dev[buf])
                shard.digest_stamps_into(self._acc[2:], lo, m)
            if self._keys is not None:                             # (the same stream point again)
                shard.row_keys(lo, m, out=self._keys)
            exported = torch.cuda.Event()
            exported.record(cur)
            self._side.wait_event(exported)
            with torch.cuda.stream(self._side):
                self._pinned[buf][:m].copy_(self._dev[buf][:m], non_blocking=True)
                if self._stamped:
                    self._gen_pinned[buf][:m].copy_(self._gen_dev[buf][:m], non_blocking=True)
                copied = torch.cuda.Event()
                copied.record(self._side)
            self._work.put(("rows", buf, lo, m, copied, None, None))
        self._cursor += m
        if self._cursor >= self._n:
            self._work.put(None)
        return True

    def pump(self):
        """Export the next chunk if a buffer is free; never blocks.  Returns True once the whole shard has been enqueued."""
        if not self.active:
            return True
        if self._cursor < self._n and self._error is None:
            self._pump_one(block=False)
        return self._cursor >= self._n

    def written(self):
        """This rank's slice is on disk (or its writer has failed: `maybe_finalize` / `finish` then raise)."""
        return self.active and self._written.is_set()

    def maybe_finalize(self, iteration):
        """At a step boundary.  Only rank-uniform conditions return before the collective: `active` (begin and finalise are collective)
        and the iteration.  Returns True when the snapshot was completed at this call."""
        if not self.active or iteration % 10 != 0:
            return False
        state = -1 if self._error is not None else (1 if self.written() else 0)
        state = self.coll.minimum(state)
        if state == 0:
            return False
        self._finalize(failed=state < 0)
        return True

    def finish(self):
        """Blocking end of the snapshot: export what is left, join the writer thread, re-raise its exception, finalise.  Collective."""
        if not self.active:
            return
        while self._cursor < self._n and self._error is None:
            self._pump_one(block=True)
        self._join()
        self._finalize(failed=self.coll.minimum(-1 if self._error is not None else 1) < 0)

    def _join(self):
        if self._cursor < self._n:                                 # a writer failed, here or on another rank: let this rank's thread end
            self._cursor = self._n
            self._work.put(None)
        self._thread.join()

    def _finalize(self, failed):
        """Steps 3 and 4 of the protocol; every rank's slice is written (or one has failed, and all raise)."""
        self._join()
        error, self.active = self._error, False
        digest = stamp_digest = None
        if not failed:
            mine, stamps = self._host_digest, self._host_stamp_digest
            if self._cuda:
                s, x, gs, gx = self._acc.tolist()                   # the one readback: everything exported has long run
                mine, stamps = (s & _MASK, x & _MASK), (gs & _MASK, gx & _MASK)
            # (also the barrier "every slice is on disk"; `_stamped` is the same on every rank, so the gather has one width everywhere)
            if self._stamped:
                digest, stamp_digest = self.coll.gather_digests(mine, stamps)
            else:
                digest = self.coll.gather_digests(mine)
        self._file = self._gen_file = self._dev = self._pinned = self._gen_dev = self._gen_pinned = None
        keys, self._keys = self._keys, None
        if failed:
            if self.coll.rank == 0:
                self._remove_parts()
            raise error if error is not None else RuntimeError("index snapshot %s failed on another rank" % self.path)
        err = None
        if self.coll.rank == 0:
            try:
                self._publish(digest, stamp_digest)
            except Exception as exc:
                err = exc
        if self.coll.minimum(0 if err is not None else 1) == 0:    # nobody returns before the meta is in place
            raise err if err is not None else RuntimeError("rank 0 could not publish %s" % self.path)
        if keys is not None:                                       # the published file is the base of the deltas from here on
            self.index.delta_base = {"keys": keys, "base": base_of(self._digest_meta(digest, stamp_digest)), "path": os.path.abspath(self.path)}
        self.log("index snapshot: %d x %d rows in %s (digest %016x %016x%s)"
                 % (self.index.num_rows, self.index.embed_size, self.path, digest[0], digest[1],
                    "" if stamp_digest is None else "; generation stamps, digest %016x %016x" % stamp_digest))

    def _remove_parts(self):
        for part in (self._tmp, stamps_path(self._tmp)):
            try:
                os.remove(part)
            except OSError:
                pass

    @staticmethod
    def _digest_meta(digest, stamp_digest=None):
        meta = {"digest_sum": "%016x" % digest[0], "digest_xor": "%016x" % digest[1]}
        if stamp_digest is not None:
            meta["stamps"] = {"digest_sum": "%016x" % stamp_digest[0], "digest_xor": "%016x" % stamp_digest[1]}
        return meta

    def _publish(self, digest, stamp_digest=None):
        from emdr2_amd.data.emdr2_index import FlatEmbeddingFile
        try:
            os.remove(meta_path(self.path))                        # from here until the new meta is written there is no valid snapshot
        except FileNotFoundError:
            pass
        flat = FlatEmbeddingFile(self._tmp)
        crc = ids_crc32(flat.ids)
        del flat
        if stamp_digest is not None:
            os.replace(stamps_path(self._tmp), stamps_path(self.path))
        else:
            try:
                os.remove(stamps_path(self.path))                  # a stale sidecar of an earlier snapshot with stamps
            except FileNotFoundError:
                pass
        remove_delta(self.path)                                    # a delta of the snapshot that is being replaced
        os.replace(self._tmp, self.path)
        meta = dict(self.meta)
        meta.update(format=SNAPSHOT_FORMAT, n=int(self.index.num_rows), dim=int(self.index.embed_size), world=int(self.coll.world), ids_crc32=crc)
        meta.update(self._digest_meta(digest, stamp_digest))
        tmp = meta_path(self.path) + '.tmp.' + _unique()
        with open(tmp, 'w') as fh:
            json.dump(meta, fh, indent=1, sort_keys=True)
            fh.write("\n")
        os.replace(tmp, meta_path(self.path))


# -- incremental snapshots -------------------------------------------------------------------------------------------------------------------
def _on_device(shard):
    return bool(getattr(shard, "tiled", None) is not None and shard.tiled.is_cuda)


def host_shard_keys(shard, lo=0, m=None):
    """The keys of rows [lo, lo + m) of a host stand-in for the shard (CPU tests), from the numpy restatement."""
    from emdr2_amd.data.emdr2_index import row_keys
    m = shard.n_rows - lo if m is None else m
    stamps = None
    if getattr(shard, "generation", None) is not None:
        stamps = np.asarray(shard.generation)[lo:lo + m]
    return row_keys(np.asarray(shard.export_rows(lo, m), dtype=np.float16), stamps, shard.row_base + lo)


def shard_keys(shard):
    """The keys of every row of the shard as it stands: a CUDA int64 tensor, or uint64 on the host for a stand-in."""
    return shard.row_keys() if _on_device(shard) else host_shard_keys(shard)


def _detect(shard, keys, cap):
    """-> (changed global rows, the first min(n_changed, cap) of them: CUDA int64 or host int64; info as 8 Python ints below 2^64)."""
    if _on_device(shard):
        rows, info = shard.changed_rows(keys, cap)
        info = [w & _MASK for w in info.tolist()]                  # the one host read
        return rows[:info[1]], info
    now = host_shard_keys(shard)
    changed = np.flatnonzero(now != keys).astype(np.int64) + shard.row_base
    stamps = shard.digest_stamps() if getattr(shard, "generation", None) is not None else (0, 0)
    first = int(changed[0]) if changed.size else _MASK
    info = [int(changed.size), min(int(changed.size), cap)] + list(shard.digest()) + list(stamps) + [first, 0]
    return changed[:info[1]], info


def save_delta(index, path, meta=None, max_fraction=0.5, log=None):
    """`DistributedBruteForceIndex.save_delta`: the protocol of the module docstring.  -> the delta's meta, or None when nothing was
    written."""
    log = log or (lambda msg: None)
    shard = index.shard
    if shard is None:
        raise RuntimeError("MIPS Index is not initialized")
    coll = _Collective(index)
    base = getattr(index, "delta_base", None)
    if base is not None and base.get("path") != os.path.abspath(path):     # (the keys of a snapshot that lives elsewhere: no base here)
        base = None
    stamped = getattr(shard, "generation", None) is not None
    n, cuda = shard.n_rows, _on_device(shard)
    cap = min(n, max(0, int(float(max_fraction) * n)))
    rows = data = stamps = None
    info = [0] * 8
    over = 0
    if base is not None:
        rows, info = _detect(shard, base["keys"], cap)
        over = int(info[0] > cap)
        if not over:                                               # the changed rows and their stamps, before anything else is enqueued
            if cuda:
                data = shard.rows_global(rows)
                stamps = shard.generation[rows - shard.row_base] if stamped else None
            else:
                local = rows - shard.row_base
                data = np.asarray(shard.export_rows(0, n), dtype=np.float16)[local]
                stamps = np.asarray(shard.generation)[local].view(np.uint32) if stamped else None
    # one all-gather: every rank sees every count, so the offsets and every decision below are rank-uniform
    words = coll.gather_words([int(base is not None), over] + info[:6])
    if not all(w[0] for w in words) or any(w[1] for w in words):
        if coll.rank == 0:
            remove_delta(path)
        coll.minimum(1)                                            # (nobody returns before the stale delta is gone)
        why = ("no base snapshot with tracked keys" if not all(w[0] for w in words) else
               "more than %g of a rank's rows changed (%s)" % (max_fraction, " ".join(str(w[2]) for w in words)))
        log("index delta: skipped, %s" % why)
        return None
    from emdr2_amd.data.emdr2_index import combine_digests
    counts = [w[2] for w in words]
    m, first = sum(counts), sum(counts[:coll.rank])
    result = combine_digests([(w[4], w[5]) for w in words])
    result_stamps = combine_digests([(w[6], w[7]) for w in words]) if stamped else None
    tmp = coll.share(delta_path(path) + '.part.' + _unique())
    err = None
    if coll.rank == 0:
        try:
            DeltaFile.create(tmp, m, index.embed_size, stamped)
        except Exception as exc:                                   # the peers are waiting: meet them first, then raise
            err = exc
    if coll.minimum(0 if err is not None else 1) == 0:
        _remove(tmp)
        raise err if err is not None else RuntimeError("rank 0 could not create %s" % tmp)
    try:
        _write_slice(DeltaFile(tmp, mode='r+'), first, rows, stamps, data, cuda)
    except BaseException as exc:
        err = exc
    if coll.minimum(0 if err is not None else 1) == 0:            # (also the barrier "every slice is on disk")
        if coll.rank == 0 or err is not None:
            _remove(tmp)
        raise err if err is not None else RuntimeError("index delta %s failed on another rank" % delta_path(path))
    out = dict(meta or {})
    if coll.rank == 0:
        try:
            _remove(delta_meta_path(path))                         # from here until the new meta is written there is no valid delta
            crc = rows_crc32(DeltaFile(tmp).rows)
            os.replace(tmp, delta_path(path))
            out.setdefault("iteration", 0)
            out.update(format=DELTA_FORMAT, m=int(m), n=int(index.num_rows), dim=int(index.embed_size), world=int(coll.world),
                       base=base["base"], result=IndexSnapshotWriter._digest_meta(result, result_stamps), rows_crc32=crc)
            part = delta_meta_path(path) + '.tmp.' + _unique()
            with open(part, 'w') as fh:
                json.dump(out, fh, indent=1, sort_keys=True)
                fh.write("\n")
            os.replace(part, delta_meta_path(path))
        except Exception as exc:
            err = exc
    if coll.minimum(0 if err is not None else 1) == 0:            # nobody returns before the meta is in place
        raise err if err is not None else RuntimeError("rank 0 could not publish %s" % delta_path(path))
    out = coll.share(out)
    log("index delta: %d of %d rows, %d bytes in %s (result digest %016x %016x%s)"
        % (m, index.num_rows, DeltaFile.layout(m, index.embed_size, stamped)[3], delta_path(path), result[0], result[1],
           "" if result_stamps is None else "; generation stamps, digest %016x %016x" % result_stamps))
    return out


def _remove(part):
    try:
        os.remove(part)
    except OSError:
        pass


def _write_slice(flat, first, rows, stamps, data, cuda):
    """This rank's changed rows into slots [first, first + len(rows)) of the delta file; from the device in chunks through one pinned buffer."""
    m = int(rows.shape[0])
    if m and cuda:
        chunk = min(m, DELTA_ROWS)
        pinned = torch.empty((chunk, data.shape[1]), dtype=torch.float16).pin_memory()
        for lo in range(0, m, chunk):
            k = min(chunk, m - lo)
            pinned[:k].copy_(data[lo:lo + k])                      # (synchronous: the buffer is read right away)
            flat.data[first + lo:first + lo + k] = pinned[:k].numpy()
        flat.rows[first:first + m] = rows.cpu().numpy()
        if stamps is not None:
            flat.stamps[first:first + m] = stamps.cpu().numpy().view(np.uint32)
    elif m:
        flat.data[first:first + m] = data
        flat.rows[first:first + m] = rows
        if stamps is not None:
            flat.stamps[first:first + m] = stamps
    flat.flush()


def apply_delta(index, path, delta_meta):
    """The delta next to the snapshot at `path` (its validated meta: `read_delta_meta`) onto the index that holds the base: every rank
    takes its slice of the ascending row list and applies it through `update_rows_at` (every derived structure stays a fresh build's),
    then the stamps; the device digests, combined over the ranks, must be the meta's `result`.  Collective; ValueError names both."""
    shard = index.shard
    flat = DeltaFile(delta_path(path))
    lo, hi = index.local_rows()
    a, b = (int(v) for v in np.searchsorted(flat.rows, [lo, hi]))
    stamped = getattr(shard, "generation", None) is not None
    cuda = _on_device(shard)
    uniform = min(max(int(delta_meta.get("iteration", 0) or 0), 0), (1 << 31) - 1)
    for at in range(a, b, DELTA_ROWS):
        k = min(DELTA_ROWS, b - at)
        rows = np.array(flat.rows[at:at + k], dtype=np.int64)
        data = np.array(flat.data[at:at + k], dtype=np.float16)
        if cuda:
            rows, data = torch.from_numpy(rows).to(shard.device), torch.from_numpy(data).to(shard.device)
        if stamped:
            index.update_rows_at(rows, data, generation=uniform)
            if flat.stamps is not None:
                shard.set_stamps_at(rows - lo, np.array(flat.stamps[at:at + k]))
        else:
            index.update_rows_at(rows, data)
    got = index_digest(index)
    want = (int(delta_meta["result"]["digest_sum"], 16), int(delta_meta["result"]["digest_xor"], 16))
    if got != want:
        raise ValueError("index delta %s: digest %016x %016x in HBM, %016x %016x in the delta's meta" % ((delta_path(path),) + got + want))
    if stamped and flat.stamps is not None and delta_meta["result"].get("stamps") is not None:
        got = index_stamp_digest(index)
        want = (int(delta_meta["result"]["stamps"]["digest_sum"], 16), int(delta_meta["result"]["stamps"]["digest_xor"], 16))
        if got != want:
            raise ValueError("index delta %s: stamp digest %016x %016x in HBM, %016x %016x in the delta's meta"
                             % ((delta_path(path),) + got + want))
