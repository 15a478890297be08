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
"""
import json
import os
import queue
import socket
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


def ids_crc32(ids):
    crc = 0
    for lo in range(0, ids.shape[0], 1 << 22):
        crc = zlib.crc32(np.ascontiguousarray(ids[lo:lo + (1 << 22)], dtype=np.int32).tobytes(), crc)
    return crc & 0xffffffff


def read_snapshot_meta(path):
    """The meta of the snapshot at `path`, validated against the data file's header -> dict.  Raises ValueError for a data file without
    a meta (an incomplete snapshot), an unknown format, or a header that disagrees; FileNotFoundError when there is no data file."""
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

    def gather_digests(self, pair):
        """This rank's (sum, xor) -> the digest over all ranks: the pairs travel as int64 bit patterns in one all-gather and are combined
        on the host mod 2^64 (an all-reduce would add int64s: signed overflow, and no XOR over every transport)."""
        from emdr2_amd.data.emdr2_index import combine_digests
        if not self.on:
            return combine_digests([pair])
        mine = torch.tensor([_to_i64(pair[0]), _to_i64(pair[1])], dtype=torch.int64, device=self.device)
        out = torch.empty((self.world * 2,), dtype=torch.int64, device=self.device)
        torch.distributed.all_gather_into_tensor(out, mine, group=self.group)
        flat = out.tolist()
        return combine_digests([(flat[2 * r] & _MASK, flat[2 * r + 1] & _MASK) for r in range(self.world)])


def index_digest(index):
    """Device digest of the whole index, combined over the ranks that share it (collective; one readback per rank)."""
    return _Collective(index).gather_digests(index.shard.digest())


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
    in rolling mode it is a mix of generations, as the live index is."""

    def __init__(self, index, chunk_rows=None, log=None):
        self.index = index
        self.chunk_rows = chunk_rows
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
        err = None
        if self.coll.rank == 0:
            try:
                FlatEmbeddingFile.create(self._tmp, index.num_rows, index.embed_size)
            except Exception as exc:                               # the peers are waiting at the barrier: meet them first, then raise
                err = exc
        if self.coll.minimum(0 if err is not None else 1) == 0:    # (also the barrier "the file exists")
            raise err if err is not None else RuntimeError("rank 0 could not create %s" % self._tmp)
        self._file = FlatEmbeddingFile(self._tmp, mode='r+')
        self._n, self._cursor = shard.n_rows, 0
        self._chunk = max(1, int(chunk_rows or self.chunk_rows or SNAPSHOT_ROWS))
        self._chunk = min(self._chunk, max(self._n, 1))
        self._cuda = bool(getattr(shard, "tiled", None) is not None and shard.tiled.is_cuda)
        self._host_digest = (0, 0)
        if self._cuda:
            self._acc = torch.zeros(2, dtype=torch.int64, device=shard.device)
            self._dev = [torch.empty((self._chunk, shard.dim), dtype=torch.float16, device=shard.device) for _ in range(2)]
            self._pinned = [torch.empty((self._chunk, shard.dim), dtype=torch.float16).pin_memory() for _ in range(2)]
            self._side = torch.cuda.Stream(device=shard.device)
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
                    return
                if self._error is not None:
                    continue
                if item[0] == "ids":
                    self._file.ids[base:base + self._n] = item[1]
                else:
                    _, buf, lo, m, event, host = item
                    if event is not None:
                        event.synchronize()
                        host = self._pinned[buf][:m].numpy()
                    self._file.rows[base + lo:base + lo + m] = host
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
            from emdr2_amd.data.emdr2_index import combine_digests
            self._host_digest = combine_digests([self._host_digest, shard.digest(lo, m)])
            self._work.put(("rows", None, lo, m, None, np.array(rows, dtype=np.float16, copy=True)))
        else:
            try:
                buf = self._free.get(block=block)
            except queue.Empty:
                return False
            cur = torch.cuda.current_stream(shard.device)
            shard.export_rows(lo, m, out=self._dev[buf])
            shard.digest_into(self._acc, lo, m)
            exported = torch.cuda.Event()
            exported.record(cur)
            self._side.wait_event(exported)
            with torch.cuda.stream(self._side):
                self._pinned[buf][:m].copy_(self._dev[buf][:m], non_blocking=True)
                copied = torch.cuda.Event()
                copied.record(self._side)
            self._work.put(("rows", buf, lo, m, copied, None))
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
        digest = None
        if not failed:
            mine = self._host_digest
            if self._cuda:
                s, x = self._acc.tolist()                           # the one readback: everything exported has long run
                mine = (s & _MASK, x & _MASK)
            digest = self.coll.gather_digests(mine)                 # (also the barrier "every slice is on disk")
        self._file = self._dev = self._pinned = None
        if failed:
            if self.coll.rank == 0:
                try:
                    os.remove(self._tmp)
                except OSError:
                    pass
            raise error if error is not None else RuntimeError("index snapshot %s failed on another rank" % self.path)
        err = None
        if self.coll.rank == 0:
            try:
                self._publish(digest)
            except Exception as exc:
                err = exc
        if self.coll.minimum(0 if err is not None else 1) == 0:    # nobody returns before the meta is in place
            raise err if err is not None else RuntimeError("rank 0 could not publish %s" % self.path)
        self.log("index snapshot: %d x %d rows in %s (digest %016x %016x)" % (self.index.num_rows, self.index.embed_size, self.path, digest[0], digest[1]))

    def _publish(self, digest):
        from emdr2_amd.data.emdr2_index import FlatEmbeddingFile
        try:
            os.remove(meta_path(self.path))                        # from here until the new meta is written there is no valid snapshot
        except FileNotFoundError:
            pass
        flat = FlatEmbeddingFile(self._tmp)
        crc = ids_crc32(flat.ids)
        del flat
        os.replace(self._tmp, self.path)
        meta = dict(self.meta)
        meta.update(format=SNAPSHOT_FORMAT, n=int(self.index.num_rows), dim=int(self.index.embed_size), world=int(self.coll.world),
                    digest_sum="%016x" % digest[0], digest_xor="%016x" % digest[1], ids_crc32=crc)
        tmp = meta_path(self.path) + '.tmp.' + _unique()
        with open(tmp, 'w') as fh:
            json.dump(meta, fh, indent=1, sort_keys=True)
            fh.write("\n")
        os.replace(tmp, meta_path(self.path))
