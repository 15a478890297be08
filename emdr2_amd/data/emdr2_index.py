"""Evidence-embedding store and MIPS index -- MI355X-native counterpart of the reference's
megatron/data/emdr2_index.py (same class and method names, same argument meaning):

  OpenRetreivalDataStore        reference emdr2_index.py:16-100   (pickle {'embed_data': {id: fp16[D]}},
                                                                    per-rank shards, merge)
  DistributedBruteForceIndex    reference emdr2_index.py:200-305  (fp16 Q*E^T + topk over all GPUs of
                                                                    ONE process)

What changes underneath: one process per GPU; every rank keeps one contiguous row shard
of the index resident in HBM in a stripe-tiled layout; `search_mips_index` runs the fused HIP scan
(libemdr2_hip.so, include/emdr2_mips.h) over the local shard for ALL queries, then ONE all-gather of
the per-shard (score, row, id) top-k over RCCL and a deterministic k-way merge on every rank.  The
dense [Q, N] score matrix of the reference is never formed.  Results follow the canonical numerics
of DESIGN.md section 3: score = RNE_fp16(exact dot), order (score desc, row asc).

There is no CPU path here: without the HIP library / a GPU the index raises.
"""
import ctypes
import os
import pickle
import shutil

import numpy as np
import torch

from emdr2_amd import _native

_UPLOAD_ROWS = 1 << 20  # rows per host->device staging chunk (1.5 GiB at D=768)


def detach(tensor):
    return tensor.detach().cpu().numpy()


class OpenRetreivalDataStore(object):
    """Serializable {doc_id -> fp16[D]} store.  Boundary kept from the reference (emdr2_index.py:16-100; the class name keeps its
    spelling): constructor arguments, `embed_data`, `add_block_data / save_shard / merge_shards_and_save / clear / load_from_file /
    state`, and the two on-disk formats -- the final pickle `{'embed_data': {id: np.float16[D]}}` at `embedding_path` and one such pickle
    per rank under `<embedding_path minus extension>_tmp/<rank>.pkl` -- so `--embedding-path` artefacts interoperate in both directions."""

    def __init__(self, embedding_path=None, load_from_path=True, rank=None):
        if embedding_path is None:                                # the reference's no-argument form: both come from the global args
            from emdr2_amd.global_vars import get_args
            embedding_path, rank = get_args().embedding_path, get_args().rank
        self.embedding_path, self.rank = embedding_path, rank
        self.temp_dir_name = os.path.splitext(embedding_path)[0] + '_tmp'
        self.embed_data = {}
        if load_from_path:
            self.load_from_file()

    # -- the serialised form ------------------------------------------------------------------------------------------------------
    def state(self):
        return {'embed_data': self.embed_data}

    @staticmethod
    def _read(path):
        with open(path, 'rb') as fh:
            return pickle.load(fh)['embed_data']

    def _write(self, path):
        # tmp + rename: a reader -- the trainers' `update_index()`, which stamps the file by size + mtime (ensure_flat_embedding_file) -- can
        # never see a half-written pickle of an indexer job that is still running
        tmp = '%s.tmp.%d' % (path, os.getpid())
        with open(tmp, 'wb') as fh:
            pickle.dump(self.state(), fh)
        os.replace(tmp, path)

    def _shard_path(self, rank):
        return os.path.join(self.temp_dir_name, '%d.pkl' % rank)

    def clear(self):
        self.embed_data = {}

    def load_from_file(self):
        self.embed_data = self._read(self.embedding_path)

    # -- filling ---------------------------------------------------------------------------------------------------------------------
    def add_block_data(self, row_id, block_embeds, allow_overwrite=False):
        """Rows are stored as fp16 whatever they arrive as (emdr2_index.py:61); re-adding an id is an error unless allowed."""
        ids = [int(i) for i in row_id]
        if not allow_overwrite:
            clash = [i for i in ids if i in self.embed_data]
            if clash or len(set(ids)) != len(ids):
                raise ValueError("Unexpectedly tried to overwrite block data")
        rows = np.asarray(block_embeds, dtype=np.float16)
        self.embed_data.update(zip(ids, rows))

    # -- per-rank shards -> one file -------------------------------------------------------------------------------------------------
    def save_shard(self):
        os.makedirs(self.temp_dir_name, exist_ok=True)
        self._write(self._shard_path(self.rank))

    def merge_shards_and_save(self):
        """Called on ONE rank after every rank's `save_shard`: fold the other ranks' shard files into this store (ids must be disjoint,
        this rank's own shard must be among the files), write the result to `embedding_path`, drop the shard directory."""
        ranks = sorted(int(os.path.splitext(name)[0]) for name in os.listdir(self.temp_dir_name))
        if self.rank not in ranks:
            raise AssertionError("merge without this rank's own shard file (%s)" % self._shard_path(self.rank))
        for r in ranks:
            if r == self.rank:
                continue
            other = self._read(self._shard_path(r))
            if not self.embed_data.keys().isdisjoint(other.keys()):
                raise AssertionError("shard %d repeats ids already merged" % r)
            self.embed_data.update(other)
        self._write(self.embedding_path)
        shutil.rmtree(self.temp_dir_name, ignore_errors=True)
        print("merged %d shard files: %d embeddings in %s" % (len(ranks), len(self.embed_data), self.embedding_path), flush=True)

    # ---- flat views (not in the reference): avoid 21M tiny arrays on the way to the GPU -----------
    def to_arrays(self):
        """(ids int32 [N], rows fp16 [N, D]) in dict insertion order == the reference's matrix row order
        (emdr2_index.py:245)."""
        n = len(self.embed_data)
        ids = np.fromiter(self.embed_data.keys(), dtype=np.int64, count=n)
        if n and (ids.min() < -2 ** 31 or ids.max() >= 2 ** 31):
            raise ValueError("doc ids must fit int32 (reference returns int32 ids, emdr2_index.py:298)")
        dim = len(next(iter(self.embed_data.values()))) if n else 0
        rows = np.empty((n, dim), dtype=np.float16)
        for lo, block in self.iter_row_blocks():
            rows[lo:lo + block.shape[0]] = block
        return ids.astype(np.int32), rows

    def iter_row_blocks(self, block_rows=1 << 18):
        """(first row, fp16 [<= block_rows, D]) blocks in dict order: the values are gathered by numpy 262,144 at a time (one C loop per
        block) instead of one Python assignment per row -- 21M of them at the full index."""
        import itertools
        it = iter(self.embed_data.values())
        lo = 0
        while True:
            chunk = list(itertools.islice(it, block_rows))
            if not chunk:
                return
            block = np.asarray(chunk, dtype=np.float16)
            if block.ndim != 2:
                raise ValueError("embedding rows of unequal length")
            yield lo, block
            lo += block.shape[0]

    def flat_path(self):
        """Where the flat twin of `embedding_path` lives (FlatEmbeddingFile; written by `ensure_flat_embedding_file`)."""
        return flat_twin_path(self.embedding_path)


# ---- flat evidence-embedding file --------------------------------------------------------------------------------
FLAT_MAGIC = b'EMDR2EMB'


# ---- row digest (include/emdr2_mips.h: emdr2_mips_digest_rows states it in full; this is its numpy restatement) -------------------
_U64 = np.uint64
_DIGEST_BLOCK_ROWS = 1 << 16


def _digest_mix(z):
    z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
    return z ^ (z >> _U64(31))


def digest_rows(rows, first_row_number=0):
    """(sum, xor) over the rows of fp16 `rows` [n, dim] of g(r), row i numbered `first_row_number + i`; Python ints below 2^64.  Bits are
    hashed, not values.  numpy on the host: an offline and test instrument (seconds per 2^18 x 768 rows), never a load path."""
    rows = np.asarray(rows)
    if rows.dtype != np.float16 or rows.ndim != 2 or rows.shape[1] % 2:
        raise ValueError("rows must be float16 [n, even dim]")
    total, x = _U64(0), _U64(0)
    tags = np.arange(1, rows.shape[1] // 2 + 1, dtype=_U64) << _U64(32)
    with np.errstate(over='ignore'):
        for lo in range(0, rows.shape[0], _DIGEST_BLOCK_ROWS):
            block = np.ascontiguousarray(rows[lo:lo + _DIGEST_BLOCK_ROWS])
            acc = _digest_mix(block.view('<u4').astype(_U64) | tags).sum(axis=1, dtype=_U64)
            number = np.arange(first_row_number + lo + 1, first_row_number + lo + 1 + block.shape[0], dtype=np.int64).astype(_U64)
            g = _digest_mix(acc ^ (number * _U64(0x9E3779B97F4A7C15)))
            total = total + g.sum(dtype=_U64)
            x = x ^ np.bitwise_xor.reduce(g)
    return int(total), int(x)


_STAMP_TAG = 0x47454E53 << 32


def digest_stamps(stamps, first_row_number=0):
    """(sum, xor) over the generation stamps `stamps` (uint32 or int32 [n], bit patterns) of h(r), stamp i belonging to row
    `first_row_number + i` -- the numpy restatement of emdr2_mips_digest_stamps (include/emdr2_mips.h); Python ints below 2^64."""
    stamps = np.asarray(stamps)
    if stamps.dtype not in (np.dtype(np.uint32), np.dtype(np.int32)) or stamps.ndim != 1:
        raise ValueError("stamps must be uint32 or int32 [n]")
    total, x = _U64(0), _U64(0)
    with np.errstate(over='ignore'):
        for lo in range(0, stamps.shape[0], 1 << 22):
            block = np.ascontiguousarray(stamps[lo:lo + (1 << 22)]).view(np.uint32).astype(_U64)
            number = np.arange(first_row_number + lo + 1, first_row_number + lo + 1 + block.shape[0], dtype=np.int64).astype(_U64)
            h = _digest_mix(_digest_mix(block | _U64(_STAMP_TAG)) ^ (number * _U64(0x9E3779B97F4A7C15)))
            total = total + h.sum(dtype=_U64)
            x = x ^ np.bitwise_xor.reduce(h)
    return int(total), int(x)


def row_keys(rows, stamps=None, first_row_number=0):
    """The per-row keys of an incremental snapshot -> uint64 [n]: g(r) of fp16 `rows` [n, dim], plus (mod 2^64) h(r) of `stamps` (uint32 or
    int32 [n]) when given, row i numbered `first_row_number + i` -- the numpy restatement of emdr2_mips_row_keys (include/emdr2_mips.h).
    Their sum and xor are `digest_rows` (+ / ^ `digest_stamps`).  A test and offline instrument, like `digest_rows`."""
    rows = np.asarray(rows)
    if rows.dtype != np.float16 or rows.ndim != 2 or rows.shape[1] % 2:
        raise ValueError("rows must be float16 [n, even dim]")
    n = rows.shape[0]
    if stamps is not None:
        stamps = np.asarray(stamps)
        if stamps.dtype not in (np.dtype(np.uint32), np.dtype(np.int32)) or stamps.shape != (n,):
            raise ValueError("stamps must be uint32 or int32 [%d]" % n)
    keys = np.empty(n, dtype=_U64)
    tags = np.arange(1, rows.shape[1] // 2 + 1, dtype=_U64) << _U64(32)
    with np.errstate(over='ignore'):
        for lo in range(0, n, _DIGEST_BLOCK_ROWS):
            block = np.ascontiguousarray(rows[lo:lo + _DIGEST_BLOCK_ROWS])
            acc = _digest_mix(block.view('<u4').astype(_U64) | tags).sum(axis=1, dtype=_U64)
            number = np.arange(first_row_number + lo + 1, first_row_number + lo + 1 + block.shape[0], dtype=np.int64).astype(_U64)
            number = number * _U64(0x9E3779B97F4A7C15)
            key = _digest_mix(acc ^ number)
            if stamps is not None:
                word = np.ascontiguousarray(stamps[lo:lo + block.shape[0]]).view(np.uint32).astype(_U64)
                key = key + _digest_mix(_digest_mix(word | _U64(_STAMP_TAG)) ^ number)
            keys[lo:lo + block.shape[0]] = key
    return keys


def combine_digests(pairs):
    """Digests of disjoint row sets -> the digest of their union: sums add mod 2^64, xors xor."""
    total, x = 0, 0
    for s, v in pairs:
        total, x = (total + int(s)) & (2 ** 64 - 1), x ^ int(v)
    return total, x


class FlatEmbeddingFile(object):
    """`[N, D]` fp16 rows + int32 doc ids in one memory-mappable file, as an alternative to the reference's pickle of N tiny arrays
    (32 GB, minutes to unpickle per reload).  Layout: 8-byte magic | u32 version = 1 | u32 D | u64 N | int32 ids[N] | pad to 4096 |
    fp16 rows[N, D].  Row order = the pickle's dict order, so an index built from either file is identical; `from_store` / `to_store`
    convert in both directions so `--embedding-path` artefacts interoperate with the reference."""

    def __init__(self, path, mode='r'):
        import struct
        self.path = path
        with open(path, 'rb') as f:
            if f.read(8) != FLAT_MAGIC:
                raise ValueError("not a flat embedding file: %s" % path)
            version, self.dim, self.n = struct.unpack('<IIQ', f.read(16))
            if version != 1:
                raise ValueError("unsupported flat embedding file version %d" % version)
        self._ids_off = 24
        self._rows_off = (self._ids_off + 4 * self.n + 4095) // 4096 * 4096
        if os.path.getsize(path) < self._rows_off + 2 * self.n * self.dim:
            raise ValueError("flat embedding file is shorter than its header says: %s" % path)
        # (numpy cannot map zero bytes: an empty file gets plain empty arrays)
        self.ids = np.memmap(path, dtype=np.int32, mode=mode, offset=self._ids_off, shape=(self.n,)) if self.n else np.empty((0,), np.int32)
        self.rows = (np.memmap(path, dtype=np.float16, mode=mode, offset=self._rows_off, shape=(self.n, self.dim)) if self.n * self.dim
                     else np.empty((self.n, self.dim), np.float16))

    @classmethod
    def create(cls, path, n, dim):
        """Header + a file of full size (zeros, sparse where the file system allows), opened WRITABLE: `ids` and `rows` are `r+` memory
        maps, so several processes -- each through its own `FlatEmbeddingFile(path, mode='r+')` -- can fill disjoint row slices.  Layout
        and version are those of `write`."""
        import struct
        n, dim = int(n), int(dim)
        with open(path, 'wb') as f:
            f.write(FLAT_MAGIC)
            f.write(struct.pack('<IIQ', 1, dim, n))
            f.truncate((24 + 4 * n + 4095) // 4096 * 4096 + 2 * n * dim)
        return cls(path, mode='r+')

    def flush(self):
        for a in (self.ids, self.rows):
            if isinstance(a, np.memmap):
                a.flush()

    def digest(self, lo=0, hi=None, row_base=None):
        """(sum, xor) digest of rows [lo, hi) as the device computes it (`HipIndexShard.digest`, emdr2_mips_digest_rows): row r of the
        file is numbered `row_base + r` (row_base None: 0, the file holds the whole index from its first row).  Blocks of 2^16 rows."""
        hi = self.n if hi is None else hi
        if not (0 <= lo <= hi <= self.n):
            raise ValueError("rows [%d, %d) are not in [0, %d]" % (lo, hi, self.n))
        return digest_rows(self.rows[lo:hi], (row_base or 0) + lo)

    @staticmethod
    def write(path, ids, rows):
        import struct
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        rows = np.ascontiguousarray(rows, dtype=np.float16)
        if rows.ndim != 2 or ids.shape != (rows.shape[0],):
            raise ValueError("ids [N] and rows [N, D] expected")
        with open(path, 'wb') as f:
            f.write(FLAT_MAGIC)
            f.write(struct.pack('<IIQ', 1, rows.shape[1], rows.shape[0]))
            f.write(ids.tobytes())
            f.write(b'\0' * ((-f.tell()) % 4096))
            f.write(rows.tobytes())

    @classmethod
    def from_store(cls, store, path):
        """Stream the store into `path` block by block (never a second dense copy of the matrix in host memory), atomically (tmp + rename)."""
        import struct
        n = len(store.embed_data)
        ids = np.fromiter(store.embed_data.keys(), dtype=np.int64, count=n)
        if n and (ids.min() < -2 ** 31 or ids.max() >= 2 ** 31):
            raise ValueError("doc ids must fit int32 (reference returns int32 ids, emdr2_index.py:298)")
        dim = len(next(iter(store.embed_data.values()))) if n else 0
        tmp = path + '.tmp.%d' % os.getpid()
        with open(tmp, 'wb') as f:
            f.write(FLAT_MAGIC)
            f.write(struct.pack('<IIQ', 1, dim, n))
            f.write(ids.astype(np.int32).tobytes())
            f.write(b'\0' * ((-f.tell()) % 4096))
            for _, block in store.iter_row_blocks():
                if block.shape[1] != dim:
                    raise ValueError("embedding rows of unequal length")
                f.write(np.ascontiguousarray(block).tobytes())
        os.replace(tmp, path)
        return cls(path)

    def to_store(self, embedding_path, rank=0):
        store = OpenRetreivalDataStore(embedding_path, load_from_path=False, rank=rank)
        store.add_block_data(self.ids.tolist(), np.asarray(self.rows))
        return store


def _node_first_rank(process_group=None):
    """True on the rank that does a node's file work -- the reference's `mpu.get_node_first_rank()` role (emdr2_model.py:414-423).  One
    process per GPU under torch.distributed.run: LOCAL_RANK 0 of every node; without a launcher's environment: rank 0 of the group."""
    dist_on = torch.distributed.is_available() and torch.distributed.is_initialized()
    if "LOCAL_RANK" in os.environ and dist_on:
        return int(os.environ["LOCAL_RANK"]) == 0
    return (torch.distributed.get_rank(process_group) if dist_on else 0) == 0


def flat_twin_path(embedding_path, cache_dir=None):
    """`<embedding_path minus extension>.flat`, or the same file name under `cache_dir` (argument, else $EMDR2_FLAT_CACHE_DIR): a node-local
    writable directory for installations whose embedding directory is read-only to the trainers (the reference needs only read access)."""
    cache_dir = cache_dir or os.environ.get("EMDR2_FLAT_CACHE_DIR")
    flat = os.path.splitext(embedding_path)[0] + '.flat'
    if cache_dir:
        os.makedirs(cache_dir, exist_ok=True)
        flat = os.path.join(cache_dir, os.path.basename(flat))
    return flat


def ensure_flat_embedding_file(embedding_path, process_group=None, log=None, cache_dir=None):
    """The flat twin of the `--embedding-path` pickle, converted ONCE per (re)load and memory-mapped by all.

    The reference unpickles the 32 GB store on the node-first rank only (emdr2_model.py:414-423) and that rank uploads every device's chunk.
    With one process per GPU every rank needs ITS rows; letting each of 8 ranks unpickle 21M small arrays and densify them costs 8 x (40 + 32)
    GB of host memory and minutes, at start-up and at every `update_index()`.  Here the FIRST RANK OF EVERY NODE (the reference's loader
    rank) converts the pickle to its flat twin if that file is missing or was made from another pickle, everybody meets at a barrier, and
    each rank then maps the file and touches only its own row range (`DistributedBruteForceIndex.add_flat_file`).  On a shared file system
    the nodes write the same bytes to private temporary files and rename them onto the one name (atomic; last writer wins, identical
    content); with `cache_dir` / $EMDR2_FLAT_CACHE_DIR the twin lives in a node-local writable directory and the embedding directory is
    only read.  A rank that finds no twin after the barrier (no node-first rank on its node reached it) converts for itself.  The pickle is
    stamped by size + mtime before AND after the conversion: a pickle replaced meanwhile (indexer jobs write tmp + rename) is converted again.
    Returns the flat file's path."""
    dist_on = torch.distributed.is_available() and torch.distributed.is_initialized()
    flat = flat_twin_path(embedding_path, cache_dir)
    side = flat + '.src'

    def stamp_of():
        st = os.stat(embedding_path)
        return "%d %d" % (st.st_size, st.st_mtime_ns)

    def fresh():
        # the twin remembers WHICH pickle it was made from (size + modification time in ns, in a sidecar): a pickle rewritten by a new
        # indexer job -- even within the same second -- makes it stale; an unchanged one is never converted twice
        try:
            with open(side) as fh:
                return os.path.exists(flat) and fh.read().strip() == stamp_of()
        except OSError:
            return False

    def convert():
        for _ in range(3):
            stamp = stamp_of()
            store = OpenRetreivalDataStore(embedding_path, load_from_path=True, rank=0)
            FlatEmbeddingFile.from_store(store, flat)
            n = len(store.embed_data)
            store.clear()
            if stamp_of() != stamp:
                continue                                          # replaced while it was being read: what was converted is already old
            tmp = '%s.tmp.%d' % (side, os.getpid())
            with open(tmp, 'w') as fh:
                fh.write(stamp)
            os.replace(tmp, side)
            if log:
                log("converted %s (%d embeddings) to %s" % (embedding_path, n, flat))
            return
        raise RuntimeError("%s kept changing while it was converted" % embedding_path)

    err = None
    if _node_first_rank(process_group):
        try:
            if not fresh():
                convert()
        except Exception as exc:                                   # the peers are waiting at the barrier: meet them first, then raise
            err = exc
    if dist_on:
        torch.distributed.barrier(process_group)
    if err is not None:
        raise err
    if not fresh():
        # a node whose first rank is not in this group / a twin directory that is not shared: convert here (what every rank of the reference's
        # one-process-per-node layout would have had to do); a missing pickle raises FileNotFoundError as an eager load would
        convert()
    return flat


def shard_bounds(num_rows, world_size):
    """Row range per rank, torch.chunk semantics like the reference's per-device split
    (emdr2_index.py:252-254): equal chunks of ceil(N/W) rows, the last one shorter (possibly empty)."""
    chunk = (num_rows + world_size - 1) // world_size if num_rows else 0
    return [(min(r * chunk, num_rows), min((r + 1) * chunk, num_rows)) for r in range(world_size)]


def resolve_duplicate_rows(row_ids):
    """int64 [n] row numbers -> a copy in which, of every value that occurs more than once, all occurrences but the LAST are -1 (which
    `HipIndexShard.update_rows_at` skips): later entries of an update list win.  Static shapes and no host read, so it runs on the
    device inside a training step; on CPU tensors too.  A stable sort keeps equal values in list order, so an element that equals its
    successor is not the last of its value; those positions receive -1 through the sort's own permutation."""
    order = torch.argsort(row_ids, stable=True)
    s = row_ids[order]
    loses = torch.zeros_like(s, dtype=torch.bool)
    loses[:-1] = s[:-1] == s[1:]
    return torch.empty_like(row_ids).scatter_(0, order, torch.where(loses, torch.full_like(s, -1), s))


def audit_result(words, shadow_in_use, nonfinite_under_shadow=None):
    """The dict `HipIndexShard.audit` / `DistributedBruteForceIndex.audit` return, from the 14 named report words of emdr2_mips_audit
    (Python ints, the first-offender words as unsigned: 2**64 - 1 = none).  `sound`: no premise of the search's proof is violated (words
    1-4 and 7-9 are zero, and no shard searches through its shadow while it holds an inf / NaN); `canonical`: every derived structure is
    bit for bit a fresh build (words 5, 6, 10, 11 are zero)."""
    out = dict(zip(_native.AUDIT_NAMES, (int(w) for w in words)))
    if nonfinite_under_shadow is None:
        nonfinite_under_shadow = bool(shadow_in_use) and out["nonfinite_rows"] > 0
    out["sound"] = all(words[i] == 0 for i in _native.AUDIT_SOUND_WORDS if i != 2) and not nonfinite_under_shadow
    out["canonical"] = all(words[i] == 0 for i in _native.AUDIT_CANONICAL_WORDS)
    out["shadow_in_use"] = bool(shadow_in_use)
    return out


def audit_failures(result):
    """One line naming the non-zero counters of an audit result and its first offenders ('' for a sound and canonical one)."""
    if result["sound"] and result["canonical"]:
        return ""
    parts = ["%s=%d" % (n, result[n]) for n in _native.AUDIT_NAMES[1:12] if result[n]]
    if result["nonfinite_rows"] and result["shadow_in_use"]:
        parts.append("(non-finite rows under a shadow in use)")
    for n in ("first_bad_row", "first_bad_block"):
        if result[n] != _native.AUDIT_NONE:
            parts.append("%s=%d" % (n, result[n]))
    return ", ".join(parts)


def generation_result(words):
    """The dict `generation_stats` returns, from the EMDR2_GEN_WORDS report words of emdr2_mips_generation_stats (Python ints): the five
    named words, `histogram` (32 bins: bin 0 = age 0, bin b = ages in [2^(b-1), 2^b)) and `mean_age` (0.0 over no rows).  `min_age` is
    2**64 - 1 when no row was covered."""
    words = [int(w) & _native.AUDIT_NONE for w in words]
    out = dict(zip(_native.GEN_NAMES, words))
    out["histogram"] = words[len(_native.GEN_NAMES):_native.GEN_WORDS]
    out["mean_age"] = out["sum_age"] / out["count"] if out["count"] else 0.0
    return out


class HipIndexShard(object):
    """One contiguous row shard resident in this process's GPU, stripe-tiled for the HIP scan.

    `shadow`: keep an int8 shadow image of the shard (+50 % HBM) and run the filter segments of at least `shadow_min_rows` rows of a
    129..512-query search on it (csrc/mips_scan8i.hip); results are bit-identical with and without.  The image is only allocated for
    shards that have such a segment, and only used while it is sealed against the current fp16 image and every row is finite.

    `generations`: keep one 32-bit stamp per local row on the device (`self.generation`; 84 MB at 21 M rows) -- the number of optimizer
    steps the weights that wrote the row had taken; every writer maintains it, the in-place writers can honour it (`newest_wins`),
    `generation_stats` reads it.  Off (the default): nothing is allocated and every entry point behaves as it always did."""

    SHADOW_MIN_ROWS = 1 << 19

    def __init__(self, dim, n_rows, row_base, device=None, shadow=True, shadow_min_rows=None, generations=False):
        self.lib = _native.lib()
        if not torch.cuda.is_available():
            raise _native.NativeError("HipIndexShard needs a GPU; there is no CPU fallback")
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.dim, self.n_rows, self.row_base = int(dim), int(n_rows), int(row_base)
        nbytes = ctypes.c_size_t()
        _native.check(self.lib.emdr2_mips_layout_bytes(max(self.n_rows, 1), self.dim, ctypes.byref(nbytes)), "layout_bytes")
        self.tiled = torch.zeros(nbytes.value, dtype=torch.uint8, device=self.device)
        self.emax_sq = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.ids = None
        self._ws = None
        self._xws = None
        self._filled = 0
        self.shadow_min_rows = int(self.SHADOW_MIN_ROWS if shadow_min_rows is None else shadow_min_rows)
        # (whether a full pass would pack the int8 query image: the search's own plan, csrc/mips_plan.h)
        self._want_shadow = bool(shadow) and self.shadow_min_rows >= 1 and _native.search_plan(self.n_rows, 512, self.dim, 1, self.shadow_min_rows)[1]
        self._shadow = None                                        # (int8 image, block table) sealed against self.tiled, or None
        self._shadow_buf = self._spare_shadow_buf = None           # their storage (kept across seals), for self.tiled / the refresh spare
        self._spare = None                                         # the second fp16 image of a swap refresh (begin_refresh)
        self._refreshing = False                                   # between begin_refresh and commit_refresh
        self._block_norms = None                                   # max ||row||^2 per 256-row block of self.tiled (update_rows), built on first use
        self._scatter_ws = None                                    # workspace of update_rows_at (claim words + touched-block list), grown on demand
        self._oldest_ws = None                                     # workspace of oldest_rows (digit histograms, per-slab counts), grown on demand
        self._delta_ws = None                                      # workspace of changed_rows (per-stripe masks, counts, digests), grown on demand
        # generation stamps of self.tiled (int32 storage of the device's uint32 words: values are below 2^31), of the refresh spare, and
        # the counter of rows that newest-wins updates left alone
        self.generation = torch.zeros(max(self.n_rows, 1), dtype=torch.int32, device=self.device) if generations else None
        self._spare_generation = None
        self._kept_newer = torch.zeros(1, dtype=torch.int32, device=self.device) if generations else None

    def _generation_of(self, generation, what):
        """a writer's `generation` argument on a shard with or without stamps -> the stamp to write (None without stamps)"""
        if self.generation is None:
            if generation:
                raise ValueError("%s: this shard keeps no generation stamps (HipIndexShard(..., generations=True))" % what)
            return None
        if generation is None:
            raise ValueError("%s on a shard with generation stamps needs generation=" % what)
        g = int(generation)
        if not 0 <= g <= _native.GEN_MAX:
            raise ValueError("generation must be in [0, 2^31)")
        return g

    def _seal(self, tiled, into):
        """Build the int8 shadow of the finished fp16 image `tiled` (on the current stream) into the buffers `into` (allocated on first
        use) -> (buffers, shadow): shadow = the buffers, or None if the shard does not take the int8 path (no long segment, or a
        non-finite row)."""
        if not self._want_shadow:
            return None, None
        if into is None:
            ib, tb = ctypes.c_size_t(), ctypes.c_size_t()
            _native.check(self.lib.emdr2_mips_shadow_bytes(self.n_rows, self.dim, ctypes.byref(ib), ctypes.byref(tb)), "shadow_bytes")
            into = (torch.empty(ib.value, dtype=torch.uint8, device=self.device), torch.empty(tb.value // 4, dtype=torch.float32, device=self.device))
        bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        _native.check(self.lib.emdr2_mips_seal_shadow(tiled.data_ptr(), self.n_rows, self.dim, into[0].data_ptr(), into[1].data_ptr(),
                                                      bad.data_ptr(), _native.stream_ptr()), "seal_shadow")
        return into, (into if int(bad.item()) == 0 else None)

    def append_rows(self, rows, generation=0):
        """rows: fp16 [n, dim] (numpy or torch, host or device); appended at the next free local row and, on a shard with stamps,
        stamped `generation` (rows loaded from a file or store: 0)."""
        generation = self._generation_of(generation, "append_rows")
        if isinstance(rows, np.ndarray):
            if rows.dtype != np.float16 or rows.ndim != 2 or rows.shape[1] != self.dim:
                raise ValueError("rows must be float16 [n, %d]" % self.dim)
        elif rows.dtype != torch.float16 or rows.dim() != 2 or rows.shape[1] != self.dim:
            raise ValueError("rows must be float16 [n, %d]" % self.dim)
        n = rows.shape[0]
        if self._filled + n > self.n_rows:
            raise ValueError("shard overflow")
        self._shadow = None
        if generation is not None and n:
            self.generation[self._filled:self._filled + n].fill_(generation)
        for lo in range(0, n, _UPLOAD_ROWS):
            chunk = rows[lo:lo + _UPLOAD_ROWS]
            if isinstance(chunk, np.ndarray):                      # (a memory map: only this 1.5 GiB piece is ever resident on the host)
                chunk = torch.from_numpy(np.array(chunk, dtype=np.float16, order='C', copy=True))
            chunk = chunk.to(self.device, non_blocking=False).contiguous()
            _native.check(self.lib.emdr2_mips_pack_rows(chunk.data_ptr(), chunk.shape[0], self.dim, self._filled,
                                                        self.n_rows, self.tiled.data_ptr(), self.emax_sq.data_ptr(),
                                                        _native.stream_ptr()), "pack_rows")
            self._filled += chunk.shape[0]
            torch.cuda.current_stream().synchronize()  # the staging chunk is released next
        if self._filled == self.n_rows:                # the shard becomes searchable: seal its shadow image
            self._shadow_buf, self._shadow = self._seal(self.tiled, self._shadow_buf)
        return self

    # -- in-HBM refresh (config 5): a second image of the shard is filled while the first keeps serving searches ---------------
    def begin_refresh(self, generation=0):
        """Allocate (once) and clear the spare stripe-tiled image; rows are then written with `refresh_rows` in any order.  One
        `generation` per pass: on a shard with stamps the spare stamp array is filled with it and swapped in by `commit_refresh` together
        with the images."""
        generation = self._generation_of(generation, "begin_refresh")
        if generation is not None:
            if self._spare_generation is None:
                self._spare_generation = torch.empty_like(self.generation)
            self._spare_generation.fill_(generation)
        if getattr(self, "_spare", None) is None:
            self._spare = torch.zeros_like(self.tiled)
            self._spare_emax = torch.zeros_like(self.emax_sq)
        else:
            self._spare.zero_(); self._spare_emax.zero_()
        self._refreshed = 0
        self._refreshing = True

    def refresh_rows(self, local_row, rows):
        """rows fp16 [n, dim] on this device -> spare image rows [local_row, local_row + n), enqueued on the CURRENT stream."""
        if rows.dtype != torch.float16 or rows.dim() != 2 or rows.shape[1] != self.dim or not rows.is_cuda:
            raise ValueError("rows must be a CUDA float16 [n, %d] tensor" % self.dim)
        n = rows.shape[0]
        if local_row < 0 or local_row + n > self.n_rows:
            raise ValueError("refresh rows out of range")
        rows = rows.contiguous()
        _native.check(self.lib.emdr2_mips_pack_rows(rows.data_ptr(), n, self.dim, local_row, self.n_rows, self._spare.data_ptr(),
                                                    self._spare_emax.data_ptr(), _native.stream_ptr()), "pack_rows")
        self._refreshed += n

    def commit_refresh(self):
        """Swap the images (the reference's `update_index`, emdr2_index.py:232-238, without the disk round trip).  The caller has made the
        searching stream wait for the stream that wrote the rows."""
        if getattr(self, "_spare", None) is None or self._refreshed != self.n_rows:
            raise RuntimeError("refresh incomplete (%d of %d rows)" % (getattr(self, "_refreshed", 0), self.n_rows))
        # (the caller's stream has waited for the rows: the seal reads the finished spare image, then the images swap)
        self._spare_shadow_buf, self._shadow = self._seal(self._spare, self._spare_shadow_buf)
        self._shadow_buf, self._spare_shadow_buf = self._spare_shadow_buf, self._shadow_buf
        self.tiled, self._spare = self._spare, self.tiled
        self.emax_sq, self._spare_emax = self._spare_emax, self.emax_sq
        if self.generation is not None:
            self.generation, self._spare_generation = self._spare_generation, self.generation
        self._refreshed = 0
        self._refreshing = False
        self._block_norms = None                                   # (it described the image that has just been swapped out)

    # -- in-place update: rows of the image that is being searched are overwritten, nothing is swapped, no second image exists ---
    def update_rows(self, local_row, rows, generation=None, newest_wins=False):
        """rows fp16 [n, dim] on this device -> rows [local_row, local_row + n) of the LIVE image, enqueued on the CURRENT stream (the
        device counterpart of the reference store's `add_block_data(..., allow_overwrite=True)`).  `emax_sq` and, when the shard has a
        sealed int8 shadow, the touched 256-row blocks of the shadow image and its table are brought to exactly what a fresh build of
        the same rows would hold (csrc: emdr2_mips_update_rows), so searches afterwards are those of a freshly built shard bit for bit.
        The caller orders the update against searches of this shard, as for `refresh_rows`: a search running concurrently on another
        stream would see a half-written block.  The block-norm table behind `emax_sq` is built on the first call (one pass over the
        image) and again after a `commit_refresh`.  If an updated block holds an inf / NaN the shard stops using its shadow until the
        next full seal, like a shard freshly built from such rows; that flag is read back with one `.item()` per call on a shard with a
        sealed shadow (a host synchronisation on the current stream -- the search that follows does one of its own).

        On a shard with stamps `generation` is required: every row written is stamped with it.  `newest_wins`: a row whose stamp is ABOVE
        `generation` is left alone, image and stamp, and counted (`kept_newer`); ties write (csrc: emdr2_mips_update_rows_stamped).  The
        result is still a fresh build of the rows the shard now holds.  On a shard without stamps both keywords raise ValueError."""
        stamp = self._stamp_of(generation, newest_wins, "update_rows")
        self._check_update_rows(rows)
        n = rows.shape[0]
        if local_row < 0 or local_row + n > self.n_rows:
            raise ValueError("update rows out of range")
        self._check_updatable()
        if n == 0:
            return
        rows = rows.contiguous()
        if stamp is not None:
            self._run_update(lambda table, shadow, image, bad: _native.check(self.lib.emdr2_mips_update_rows_stamped(
                rows.data_ptr(), n, self.dim, local_row, self.n_rows, self.tiled.data_ptr(), table.data_ptr(), self.emax_sq.data_ptr(), shadow, image,
                bad, *stamp, _native.stream_ptr()), "update_rows_stamped"))
            return
        self._run_update(lambda table, shadow, image, bad: _native.check(self.lib.emdr2_mips_update_rows(
            rows.data_ptr(), n, self.dim, local_row, self.n_rows, self.tiled.data_ptr(), table.data_ptr(), self.emax_sq.data_ptr(), shadow, image, bad,
            _native.stream_ptr()), "update_rows"))

    def update_rows_at(self, local_rows, rows, generation=None, newest_wins=False):
        """`update_rows` addressed by a list: rows fp16 [n, dim] and local_rows int64 [n], both on this device; entry i goes to row
        local_rows[i] of the LIVE image (csrc: emdr2_mips_update_rows_scattered).  Entries outside [0, n_rows) are skipped, so a list
        that also names rows of other shards needs no compaction.  Where a row is named more than once the LAST occurrence wins
        (`resolve_duplicate_rows`, on the device, no host read).  Same preconditions, same result and same non-finite read-back as
        `update_rows`: afterwards the shard is byte for byte a fresh build of the same rows.  `generation` / `newest_wins` as for
        `update_rows` (csrc: emdr2_mips_update_rows_scattered_stamped): duplicates are resolved first, the stamp rule then applies to the
        surviving entry; skipped entries are never counted as kept newer."""
        stamp = self._stamp_of(generation, newest_wins, "update_rows_at")
        self._check_update_rows(rows)
        if local_rows.dtype != torch.int64 or local_rows.dim() != 1 or not local_rows.is_cuda:
            raise ValueError("local_rows must be a CUDA int64 [n] tensor")
        n = rows.shape[0]
        if local_rows.shape[0] != n:
            raise ValueError("%d row numbers for %d rows" % (local_rows.shape[0], n))
        self._check_updatable()
        if n == 0:
            return
        rows = rows.contiguous()
        ids = resolve_duplicate_rows(local_rows.contiguous())
        nbytes = ctypes.c_size_t()
        _native.check(self.lib.emdr2_mips_scatter_workspace_bytes(self.n_rows, n, ctypes.byref(nbytes)), "scatter_workspace_bytes")
        if self._scatter_ws is None or self._scatter_ws.numel() < nbytes.value:
            self._scatter_ws = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        ws = self._scatter_ws
        if stamp is not None:
            self._run_update(lambda table, shadow, image, bad: _native.check(self.lib.emdr2_mips_update_rows_scattered_stamped(
                rows.data_ptr(), ids.data_ptr(), n, self.dim, self.n_rows, self.tiled.data_ptr(), table.data_ptr(), self.emax_sq.data_ptr(), shadow,
                image, bad, ws.data_ptr(), ws.numel(), *stamp, _native.stream_ptr()), "update_rows_scattered_stamped"))
            return
        self._run_update(lambda table, shadow, image, bad: _native.check(self.lib.emdr2_mips_update_rows_scattered(
            rows.data_ptr(), ids.data_ptr(), n, self.dim, self.n_rows, self.tiled.data_ptr(), table.data_ptr(), self.emax_sq.data_ptr(), shadow, image,
            bad, ws.data_ptr(), ws.numel(), _native.stream_ptr()), "update_rows_scattered"))

    def _stamp_of(self, generation, newest_wins, what):
        """the four stamp arguments of the stamped entry points, or None on a shard without stamps (where the keywords are refused)"""
        if self.generation is None:
            if generation is not None or newest_wins:
                raise ValueError("%s: generation / newest_wins need a shard with generation stamps (HipIndexShard(..., generations=True))" % what)
            return None
        g = self._generation_of(generation, what)
        return self.generation.data_ptr(), g, int(bool(newest_wins)), self._kept_newer.data_ptr()

    def kept_newer(self):
        """Rows that newest-wins updates have left alone since the last call: reads and clears the device counter.  ONE host read, so it is
        only called where a log line is printed."""
        if self.generation is None:
            raise ValueError("this shard keeps no generation stamps")
        n = int(self._kept_newer.item())
        self._kept_newer.zero_()
        return n

    def generation_report(self, now, global_rows=None):
        """`generation_stats` without the host read: the report of emdr2_mips_generation_stats as CUDA int64 [GEN_WORDS] (bit patterns of
        the uint64 words), enqueued on the current stream."""
        if self.generation is None:
            raise ValueError("this shard keeps no generation stamps")
        now = int(now)
        if not 0 <= now < (1 << 32):
            raise ValueError("now must be in [0, 2^32)")
        report = torch.empty(_native.GEN_WORDS, dtype=torch.int64, device=self.device)
        rows_ptr, n_sel = None, 0
        if global_rows is not None:
            if not torch.is_tensor(global_rows) or global_rows.dtype != torch.int64 or global_rows.device != self.device:
                raise ValueError("global_rows must be an int64 tensor on %s" % (self.device,))
            global_rows = global_rows.contiguous()
            rows_ptr, n_sel = global_rows.data_ptr(), global_rows.numel()
        n_rows = self._filled if self._filled == self.n_rows else 0          # (a shard still being filled has no rows to report)
        if global_rows is not None and n_sel == 0:
            rows_ptr, n_rows = None, 0                                        # (an empty tensor has no pointer to tell "no list" from "an empty list")
        _native.check(self.lib.emdr2_mips_generation_stats(self.generation.data_ptr(), n_rows, self.row_base, rows_ptr, n_sel, now,
                                                           report.data_ptr(), _native.stream_ptr()), "generation_stats")
        return report

    def generation_stats(self, now, global_rows=None):
        """Ages of this shard's rows at step count `now` (age = now - stamp, 0 where the stamp exceeds `now`): of all rows of the image
        being searched, or of the entries of `global_rows` (CUDA int64 of any shape, e.g. `last_search_rows`) that fall into this shard --
        -1 and other shards' rows are not counted, a row named twice counts twice.  One pass on the device, then ONE host read of the
        296-byte report -> dict (`generation_result`)."""
        return generation_result(self.generation_report(now, global_rows).tolist())

    def oldest_rows(self, n, below):
        """The `n` oldest rows of this shard among those stamped below `below` (csrc: emdr2_mips_oldest_rows) -> (rows, info): `rows`
        CUDA int64 [n], the selected GLOBAL rows in ascending row order, -1 in every slot behind them; `info` CUDA int64 [4]: rows
        selected, rows eligible (stamp < below), the largest stamp selected (-1: none), 0.  The oldest stamps first, the lowest rows
        first among equal stamps -- so on a shard with uniform stamps below `below` the result is the first n rows.  `n` is clamped to
        the shard's rows.  Enqueued on the current stream, no host read; the caller orders it against the writers of the stamps.
        ValueError on a shard without stamps or still being filled, and for `below` outside [0, 2^31]."""
        if self.generation is None:
            raise ValueError("this shard keeps no generation stamps")
        if self._filled != self.n_rows:
            raise ValueError("shard not fully populated (%d of %d rows)" % (self._filled, self.n_rows))
        n, below = int(n), int(below)
        if n < 0:
            raise ValueError("n must be >= 0")
        if not 0 <= below <= _native.GEN_MAX + 1:
            raise ValueError("below must be in [0, 2^31]")
        n = min(n, self.n_rows)
        nbytes = ctypes.c_size_t()
        _native.check(self.lib.emdr2_mips_oldest_rows_workspace_bytes(self.n_rows, ctypes.byref(nbytes)), "oldest_rows_workspace_bytes")
        if self._oldest_ws is None or self._oldest_ws.numel() < nbytes.value:
            self._oldest_ws = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        ws = self._oldest_ws
        rows = torch.empty(n, dtype=torch.int64, device=self.device)
        info = torch.empty(4, dtype=torch.int64, device=self.device)
        _native.check(self.lib.emdr2_mips_oldest_rows(self.generation.data_ptr(), self.n_rows, self.row_base, below, n,
                                                      rows.data_ptr() if n else None, info.data_ptr(), ws.data_ptr(), ws.numel(),
                                                      _native.stream_ptr()), "oldest_rows")
        return rows, info

    def _check_update_rows(self, rows):
        if rows.dtype != torch.float16 or rows.dim() != 2 or rows.shape[1] != self.dim or not rows.is_cuda:
            raise ValueError("rows must be a CUDA float16 [n, %d] tensor" % self.dim)

    def _check_updatable(self):
        if self._filled != self.n_rows:
            raise RuntimeError("shard not fully populated (%d of %d rows)" % (self._filled, self.n_rows))
        if self._refreshing:
            raise RuntimeError("a swap refresh is in progress (begin_refresh without commit_refresh): its commit would discard the update")

    def _run_update(self, call):
        """What both in-place updates share: the block-norm table (built on first use), the sealed shadow's pointers and the read-back of
        the non-finite flag.  call(table, shadow image ptr, shadow table ptr, flag ptr) enqueues the update itself."""
        if self._block_norms is None:
            nbytes = ctypes.c_size_t()
            _native.check(self.lib.emdr2_mips_block_norm_bytes(self.n_rows, ctypes.byref(nbytes)), "block_norm_bytes")
            table = torch.empty(nbytes.value // 4, dtype=torch.float32, device=self.device)
            _native.check(self.lib.emdr2_mips_block_norms(self.tiled.data_ptr(), self.n_rows, self.dim, 0, table.numel(), table.data_ptr(),
                                                          _native.stream_ptr()), "block_norms")
            self._block_norms = table
        shadow = self._shadow
        if shadow is None:
            call(self._block_norms, None, None, None)
            return
        bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        call(self._block_norms, shadow[0].data_ptr(), shadow[1].data_ptr(), bad.data_ptr())
        if int(bad.item()) != 0:
            self._shadow = None

    def set_ids(self, ids):
        ids = torch.as_tensor(np.ascontiguousarray(ids, dtype=np.int32)) if not torch.is_tensor(ids) else ids.to(torch.int32)
        if ids.numel() != self.n_rows:
            raise ValueError("ids must have one entry per shard row")
        self.ids = ids.to(self.device).contiguous()

    def _workspace(self, k):
        if self._ws is None:
            nbytes = ctypes.c_size_t()
            _native.check(self.lib.emdr2_mips_workspace_bytes(512, self.dim, k, ctypes.byref(nbytes)), "workspace_bytes")
            self._ws = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        return self._ws

    def _search(self, queries, k, f32, rec, exact_fallback=True, out=None):
        """The one search.  `rec` False: the fast path into three arrays (dist fp16, or fp32 when `f32`) -> (dist, idx, row, flags).
        `rec` True: into a records buffer (`out`, or a new one) -> (records, flags).  Then the all-exact path for the queries the fast
        path flagged (one host sync, like the reference's .item() loop), their records re-packed."""
        if self._filled != self.n_rows:
            raise RuntimeError("shard not fully populated (%d of %d rows)" % (self._filled, self.n_rows))
        if queries.dtype != torch.float16 or queries.dim() != 2 or queries.shape[1] != self.dim or not queries.is_cuda:
            raise ValueError("queries must be a CUDA float16 [Q, %d] tensor" % self.dim)
        if not (1 <= k <= _native.MAX_TOPK):
            raise ValueError("top_k must be in [1, %d]" % _native.MAX_TOPK)
        q = queries.contiguous()
        nq = q.shape[0]
        rec = (out if out is not None else torch.empty((nq, k, 16), dtype=torch.uint8, device=self.device)) if rec else None
        if rec is not None and (rec.shape != (nq, k, 16) or rec.dtype != torch.uint8 or not rec.is_contiguous()):
            raise ValueError("records buffer must be a contiguous uint8 [Q, k, 16] tensor")

        def arrays():
            return (torch.empty((nq, k), dtype=torch.float32 if f32 else torch.float16, device=self.device),
                    torch.empty((nq, k), dtype=torch.int32, device=self.device), torch.empty((nq, k), dtype=torch.int64, device=self.device))
        dist, idx, row = arrays() if rec is None else (None, None, None)
        # (the search's init launch clears the flags of all nq queries: no fill launch of their own)
        flags = torch.empty((nq,), dtype=torch.int32, device=self.device)
        if self.n_rows == 0:
            flags.zero_()
            if rec is None:
                dist.fill_(float('-inf')); idx.fill_(-1); row.fill_(-1)
            else:
                rec.view(torch.int32).copy_(torch.tensor([-1, -1, -1, 0xff800000 - (1 << 32) if f32 else 0xfc00], dtype=torch.int32, device=self.device))
            return (dist, idx, row, flags) if rec is None else (rec, flags)
        ws = self._workspace(k)
        ptr = lambda t: None if t is None else t.data_ptr()
        head = (self.tiled.data_ptr(), self.n_rows, self.dim, self.row_base, self.emax_sq.data_ptr())
        tail = (flags.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_ptr())
        if self._shadow is not None:                                # the long filter segments on the sealed int8 shadow image
            _native.check(self.lib.emdr2_mips_search_shadow(*head, self._shadow[0].data_ptr(), self._shadow[1].data_ptr(), self.shadow_min_rows,
                                                            q.data_ptr(), nq, k, ptr(self.ids), int(f32), ptr(dist), ptr(idx), ptr(row), ptr(rec),
                                                            *tail), "mips_search_shadow")
        elif rec is not None:
            _native.check(self.lib.emdr2_mips_search_records(*head, q.data_ptr(), nq, k, ptr(self.ids), int(f32), rec.data_ptr(), *tail),
                          "mips_search_records")
        else:
            fn, what = (self.lib.emdr2_mips_search_f32, "mips_search_f32") if f32 else (self.lib.emdr2_mips_search, "mips_search")
            _native.check(fn(*head, q.data_ptr(), nq, k, ptr(self.ids), dist.data_ptr(), idx.data_ptr(), row.data_ptr(), *tail), what)
        if exact_fallback:
            sel = torch.nonzero(flags).to(torch.int32).flatten()
            if sel.numel():
                sel = sel.contiguous()
                if rec is not None:
                    dist, idx, row = arrays()
                self.search_exact(q, sel, k, dist, idx, row, flags, f32)
                if rec is not None:
                    _native.check(self.lib.emdr2_mips_pack_records(dist.data_ptr(), idx.data_ptr(), row.data_ptr(), sel.data_ptr(), int(sel.numel()),
                                                                   k, int(f32), rec.data_ptr(), _native.stream_ptr()), "mips_pack_records")
        return (dist, idx, row, flags) if rec is None else (rec, flags)

    def search(self, queries, k, exact_fallback=True):
        """queries fp16 [Q, dim] on this device -> (dist fp16 [Q,k], idx int32, row int64, flags uint32-as-int32)."""
        return self._search(queries, k, False, False, exact_fallback)

    def search_f32(self, queries, k, exact_fallback=True):
        """FaissMIPSIndex-style scores: queries fp16 [Q, dim] -> (dist fp32 [Q,k] = RNE_fp32(exact dot), idx int32, row int64, flags),
        order (fp32 score desc, row asc)."""
        return self._search(queries, k, True, False, exact_fallback)

    def search_records(self, queries, k, f32=False, out=None, exact_fallback=True):
        """The shard's canonical top-k as ONE uint8 [Q, k, 16] tensor of packed records {int64 global row | int32 doc id | score bits}
        (include/emdr2_mips.h) -- what a sharded search puts into its all-gather: `out` may be the send buffer itself.  Queries the fast
        path flags are re-done by the all-exact path and their records overwritten (one host sync, as in `search`).  -> (records, flags)."""
        return self._search(queries, k, bool(f32), True, exact_fallback, out)

    def search_exact(self, q, sel, k, dist, idx, row, flags, f32=False):
        """The all-exact path for queries sel (int32 indices into q): their rows of dist (fp16, or fp32 when `f32`) / idx / row are
        overwritten with the canonical top-k and their flags cleared."""
        suffix = "_f32" if f32 else ""
        nbytes = ctypes.c_size_t()
        _native.check(getattr(self.lib, "emdr2_mips_exact_workspace_bytes" + suffix)(self.n_rows, int(sel.numel()), ctypes.byref(nbytes)),
                      "exact_workspace_bytes" + suffix)
        if self._xws is None or self._xws.numel() < nbytes.value:
            self._xws = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        ids_ptr = self.ids.data_ptr() if self.ids is not None else None
        sel = sel.contiguous()
        _native.check(getattr(self.lib, "emdr2_mips_search_exact" + suffix)(
            self.tiled.data_ptr(), self.n_rows, self.dim, self.row_base, q.data_ptr(), q.shape[0], sel.data_ptr(), int(sel.numel()), k, ids_ptr,
            dist.data_ptr(), idx.data_ptr(), row.data_ptr(), flags.data_ptr(), self._xws.data_ptr(), self._xws.numel(), _native.stream_ptr()),
            "mips_search_exact" + suffix)

    def debug_scores(self, queries):
        q = queries.contiguous()
        out = torch.empty((q.shape[0], self.n_rows), dtype=torch.float32, device=self.device)
        ws = self._workspace(50)
        _native.check(self.lib.emdr2_mips_debug_scores(self.tiled.data_ptr(), self.n_rows, self.dim, q.data_ptr(), q.shape[0],
                                                       out.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_ptr()), "debug_scores")
        return out

    def rows(self, local_row_ids):
        r = torch.as_tensor(local_row_ids, dtype=torch.int64, device=self.device).contiguous()
        out = torch.empty((r.numel(), self.dim), dtype=torch.float16, device=self.device)
        _native.check(self.lib.emdr2_mips_unpack_rows(self.tiled.data_ptr(), self.n_rows, self.dim, r.data_ptr(), r.numel(),
                                                      out.data_ptr(), _native.stream_ptr()), "unpack_rows")
        return out

    def rows_global(self, global_rows, out=None):
        """Rows of the LIVE image (during a swap-mode refresh: the image being searched, not the spare) addressed by GLOBAL row, as a search
        returns them: CUDA int64 of any shape [...] -> fp16 [..., dim], enqueued on the current stream (csrc: emdr2_mips_gather_rows).  A
        row outside this shard's [row_base, row_base + n_rows) -- -1, another rank's row, the padding -- comes back as zeros, so every
        rank can be handed the same merged list.  `out`: a contiguous CUDA fp16 buffer of that shape to write into.  Ordered against
        in-place updates like a search: the caller orders it."""
        if not torch.is_tensor(global_rows) or global_rows.dtype != torch.int64 or global_rows.device != self.device:
            raise ValueError("global_rows must be an int64 tensor on %s" % (self.device,))
        r = global_rows.contiguous()
        shape = tuple(r.shape) + (self.dim,)
        if out is None:
            out = torch.empty(shape, dtype=torch.float16, device=self.device)
        elif out.dtype != torch.float16 or tuple(out.shape) != shape or out.device != self.device or not out.is_contiguous():
            raise ValueError("out must be a contiguous CUDA float16 %s tensor" % (shape,))
        if r.numel():
            _native.check(self.lib.emdr2_mips_gather_rows(self.tiled.data_ptr(), self.n_rows, self.dim, self.row_base, r.data_ptr(), r.numel(),
                                                          out.data_ptr(), _native.stream_ptr()), "gather_rows")
        return out

    # -- audit: the premises of the search's proof, re-checked on the live image (emdr2_mips_audit) -------------------
    def audit(self):
        """One streaming pass over the image this shard is SEARCHING (between `begin_refresh` and `commit_refresh` that is the old image,
        not the spare), its int8 shadow when one is in use, `emax_sq` and -- if an in-place update has built it -- the block-norm table;
        enqueued on the current stream and ordered like a search, then ONE host read of the 128-byte report.  -> dict of the named report
        words (include/emdr2_mips.h) plus `sound`, `canonical`, `shadow_in_use` (`audit_result`).  Nothing is built and nothing repaired."""
        if self._filled != self.n_rows:
            raise RuntimeError("shard not fully populated (%d of %d rows)" % (self._filled, self.n_rows))
        report = torch.empty(_native.AUDIT_WORDS, dtype=torch.int64, device=self.device)
        shadow, norms = self._shadow, self._block_norms
        _native.check(self.lib.emdr2_mips_audit(self.tiled.data_ptr(), self.n_rows, self.dim, self.row_base, self.emax_sq.data_ptr(),
                                                None if norms is None else norms.data_ptr(), None if shadow is None else shadow[0].data_ptr(),
                                                None if shadow is None else shadow[1].data_ptr(), report.data_ptr(), _native.stream_ptr()),
                      "mips_audit")
        words = [w & _native.AUDIT_NONE for w in report.tolist()]
        return audit_result(words[:len(_native.AUDIT_NAMES)], shadow is not None)

    # -- snapshots: the way out of HBM (emdr2_mips_export_rows / _digest_rows) ---------------------------------------------------------
    def _check_range(self, local_row, n):
        if self._filled != self.n_rows:
            raise RuntimeError("shard not fully populated (%d of %d rows)" % (self._filled, self.n_rows))
        if local_row < 0 or n < 0 or local_row + n > self.n_rows:
            raise ValueError("rows [%d, %d) are not in this shard's [0, %d)" % (local_row, local_row + n, self.n_rows))

    def export_rows(self, local_row, n, out=None):
        """Rows [local_row, local_row + n) of the LIVE image as row-major CUDA fp16 [n, dim], enqueued on the current stream -- the inverse
        of `append_rows` for a contiguous range, without a row-id array.  `out`: a contiguous CUDA fp16 buffer of at least n rows to
        write into (its first n rows are returned)."""
        local_row, n = int(local_row), int(n)
        self._check_range(local_row, n)
        if out is None:
            out = torch.empty((n, self.dim), dtype=torch.float16, device=self.device)
        elif out.dtype != torch.float16 or out.dim() != 2 or out.shape[1] != self.dim or out.shape[0] < n or not out.is_cuda or not out.is_contiguous():
            raise ValueError("out must be a contiguous CUDA float16 [>= %d, %d] tensor" % (n, self.dim))
        out = out[:n]
        if n:
            _native.check(self.lib.emdr2_mips_export_rows(self.tiled.data_ptr(), self.n_rows, self.dim, local_row, n, out.data_ptr(),
                                                          _native.stream_ptr()), "export_rows")
        return out

    def digest_into(self, acc, local_row=0, n=None):
        """Fold the digest of rows [local_row, local_row + n) into `acc` (CUDA int64 [2], zeroed by the caller: the bit patterns of the
        uint64 sum and xor) on the current stream; no readback.  Rows are numbered `row_base + local row`."""
        n = self.n_rows - local_row if n is None else int(n)
        self._check_range(int(local_row), n)
        if acc.dtype != torch.int64 or acc.numel() != 2 or not acc.is_cuda or not acc.is_contiguous():
            raise ValueError("acc must be a contiguous CUDA int64 [2] tensor")
        if n:
            _native.check(self.lib.emdr2_mips_digest_rows(self.tiled.data_ptr(), self.n_rows, self.dim, int(local_row), n, self.row_base,
                                                          acc.data_ptr(), _native.stream_ptr()), "digest_rows")
        return acc

    def digest(self, local_row=0, n=None):
        """(sum, xor) digest of rows [local_row, local_row + n) of the live image (default: the whole shard) as Python ints; equals
        `FlatEmbeddingFile.digest` of the same rows under the same numbering.  One readback."""
        acc = self.digest_into(torch.zeros(2, dtype=torch.int64, device=self.device), local_row, n)
        s, x = acc.tolist()
        return s & (2 ** 64 - 1), x & (2 ** 64 - 1)

    # -- the stamps' way out of HBM and back (emdr2_mips_digest_stamps); every call reads `self.generation` as it stands: commit_refresh swaps it
    def _check_stamp_range(self, local_row, n):
        if self.generation is None:
            raise ValueError("this shard keeps no generation stamps")
        self._check_range(local_row, n)

    def export_stamps(self, local_row, n, out=None):
        """The stamps of rows [local_row, local_row + n) as CUDA int32 [n] (the storage of the device's uint32 words), copied on the
        current stream.  `out`: a contiguous CUDA int32 buffer of at least n words to write into (its first n are returned)."""
        local_row, n = int(local_row), int(n)
        self._check_stamp_range(local_row, n)
        if out is None:
            out = torch.empty(n, dtype=torch.int32, device=self.device)
        elif out.dtype != torch.int32 or out.dim() != 1 or out.shape[0] < n or not out.is_cuda or not out.is_contiguous():
            raise ValueError("out must be a contiguous CUDA int32 [>= %d] tensor" % n)
        out = out[:n]
        if n:
            out.copy_(self.generation[local_row:local_row + n])
        return out

    def digest_stamps_into(self, acc, local_row=0, n=None):
        """Fold the digest of the stamps of rows [local_row, local_row + n) into `acc` (CUDA int64 [2], zeroed by the caller) on the
        current stream; no readback.  Rows are numbered `row_base + local row`, as for `digest_into`."""
        n = self.n_rows - local_row if n is None else int(n)
        self._check_stamp_range(int(local_row), n)
        if acc.dtype != torch.int64 or acc.numel() != 2 or not acc.is_cuda or not acc.is_contiguous():
            raise ValueError("acc must be a contiguous CUDA int64 [2] tensor")
        if n:
            _native.check(self.lib.emdr2_mips_digest_stamps(self.generation.data_ptr(), self.n_rows, int(local_row), n, self.row_base,
                                                            acc.data_ptr(), _native.stream_ptr()), "digest_stamps")
        return acc

    def digest_stamps(self, local_row=0, n=None):
        """(sum, xor) digest of the stamps of rows [local_row, local_row + n) (default: the whole shard) as Python ints; equals the
        host `digest_stamps` of the same stamps under the same numbering.  One readback."""
        acc = self.digest_stamps_into(torch.zeros(2, dtype=torch.int64, device=self.device), local_row, n)
        s, x = acc.tolist()
        return s & (2 ** 64 - 1), x & (2 ** 64 - 1)

    def set_stamps(self, local_row, stamps):
        """`stamps` (host uint32 or int32 [n], every value below 2^31) -> the stamps of rows [local_row, local_row + n) of the live image
        (a snapshot's sidecar, after its rows are in).  The copy is enqueued on the current stream."""
        stamps = np.ascontiguousarray(stamps)
        if stamps.dtype not in (np.dtype(np.uint32), np.dtype(np.int32)) or stamps.ndim != 1:
            raise ValueError("stamps must be a host uint32 or int32 [n] array")
        local_row, n = int(local_row), stamps.shape[0]
        self._check_stamp_range(local_row, n)
        if n == 0:
            return
        if int(stamps.view(np.uint32).max()) > _native.GEN_MAX:
            raise ValueError("generation stamps must be below 2^31")
        self.generation[local_row:local_row + n].copy_(torch.from_numpy(np.array(stamps.view(np.int32), copy=True)))

    def set_stamps_at(self, local_rows, stamps):
        """A scattered `set_stamps`: `stamps` (host uint32 or int32 [n], every value below 2^31) -> the stamps of the rows `local_rows`
        (int64 [n], host or this device; every entry in [0, n_rows), no row named twice) -- an incremental snapshot's stamps, after its
        rows are in.  One indexed copy, enqueued on the current stream."""
        stamps = np.ascontiguousarray(stamps)
        if stamps.dtype not in (np.dtype(np.uint32), np.dtype(np.int32)) or stamps.ndim != 1:
            raise ValueError("stamps must be a host uint32 or int32 [n] array")
        local_rows = torch.as_tensor(local_rows)
        if local_rows.dtype != torch.int64 or local_rows.dim() != 1 or local_rows.shape[0] != stamps.shape[0]:
            raise ValueError("local_rows must be int64 [%d]" % stamps.shape[0])
        self._check_stamp_range(0, 0)
        if stamps.shape[0] == 0:
            return
        if int(stamps.view(np.uint32).max()) > _native.GEN_MAX:
            raise ValueError("generation stamps must be below 2^31")
        if not local_rows.is_cuda and (int(local_rows.min()) < 0 or int(local_rows.max()) >= self.n_rows):
            raise ValueError("local_rows outside this shard's [0, %d)" % self.n_rows)
        values = torch.from_numpy(np.array(stamps.view(np.int32), copy=True)).to(self.device)
        self.generation.index_copy_(0, local_rows.to(self.device), values)

    # -- incremental snapshots: per-row keys and the rows whose key differs from a base's (emdr2_mips_row_keys / _changed_rows) ------------
    def row_keys(self, local_row=0, n=None, out=None):
        """The keys of rows [local_row, local_row + n) of the live image (default: the whole shard): g(r), plus h(r) on a shard with
        stamps -- the host `row_keys` of the same rows and stamps, bit for bit.  -> CUDA int64 [n_rows] (the uint64 keys' bit patterns)
        whose slots [local_row, local_row + n) have been written on the current stream; `out`: such a tensor to write into (the other
        slots are left alone; without `out` they are uninitialised)."""
        local_row = int(local_row)
        n = self.n_rows - local_row if n is None else int(n)
        self._check_range(local_row, n)
        if out is None:
            out = torch.empty(self.n_rows, dtype=torch.int64, device=self.device)
        elif out.dtype != torch.int64 or out.dim() != 1 or out.shape[0] != self.n_rows or out.device != self.device or not out.is_contiguous():
            raise ValueError("out must be a contiguous CUDA int64 [%d] tensor" % self.n_rows)
        if n:
            _native.check(self.lib.emdr2_mips_row_keys(self.tiled.data_ptr(), self.n_rows, self.dim, local_row, n, self.row_base,
                                                       None if self.generation is None else self.generation.data_ptr(), out.data_ptr(),
                                                       _native.stream_ptr()), "row_keys")
        return out

    def changed_rows(self, base_keys, cap):
        """The rows of this shard whose key differs from `base_keys` (CUDA int64 [n_rows], as `row_keys` gave them for a base snapshot;
        read, never written) -> (rows, info): `rows` CUDA int64 [cap], the changed GLOBAL rows in ascending order, the first `cap` of
        them, -1 in every slot behind; `info` CUDA int64 [8] (bit patterns of uint64 words): rows changed, rows stored, the (sum, xor)
        of `digest()` and of `digest_stamps()` (0, 0 without stamps) of the whole shard at this stream point, the smallest changed global
        row (-1: none), 0.  One pass over the image and two small launches on the current stream, no host read; the caller orders it
        against the shard's writers.  `cap` is clamped to the shard's rows.  A shard being filled or refreshed is refused."""
        if self._filled != self.n_rows:
            raise ValueError("shard not fully populated (%d of %d rows)" % (self._filled, self.n_rows))
        if self._refreshing:
            raise ValueError("a swap refresh is in progress (begin_refresh without commit_refresh): the live image is about to be replaced")
        if (not torch.is_tensor(base_keys) or base_keys.dtype != torch.int64 or base_keys.dim() != 1 or base_keys.shape[0] != self.n_rows
                or base_keys.device != self.device or not base_keys.is_contiguous()):
            raise ValueError("base_keys must be a contiguous CUDA int64 [%d] tensor" % self.n_rows)
        cap = int(cap)
        if cap < 0:
            raise ValueError("cap must be >= 0")
        cap = min(cap, self.n_rows)
        nbytes = ctypes.c_size_t()
        _native.check(self.lib.emdr2_mips_changed_rows_workspace_bytes(self.n_rows, ctypes.byref(nbytes)), "changed_rows_workspace_bytes")
        if self._delta_ws is None or self._delta_ws.numel() < nbytes.value:
            self._delta_ws = torch.empty(max(nbytes.value, 16), dtype=torch.uint8, device=self.device)
        ws = self._delta_ws
        rows = torch.empty(cap, dtype=torch.int64, device=self.device)
        info = torch.empty(8, dtype=torch.int64, device=self.device)
        _native.check(self.lib.emdr2_mips_changed_rows(self.tiled.data_ptr(), self.n_rows, self.dim, self.row_base,
                                                       None if self.generation is None else self.generation.data_ptr(),
                                                       base_keys.data_ptr() if self.n_rows else None, cap, rows.data_ptr() if cap else None,
                                                       info.data_ptr(), ws.data_ptr(), ws.numel(), _native.stream_ptr()), "changed_rows")
        return rows, info


def merge_shard_results(dist, idx, row):
    """[S, Q, k] per-shard canonical lists (device; dist fp16, or fp32 for the FaissMIPSIndex-style scores) -> merged [Q, k] via the HIP
    merge kernel."""
    lib = _native.lib()
    s, nq, k = dist.shape
    f32 = dist.dtype == torch.float32
    if not f32 and dist.dtype != torch.float16:
        raise ValueError("dist must be float16 or float32")
    od = torch.empty((nq, k), dtype=dist.dtype, device=dist.device)
    oi = torch.empty((nq, k), dtype=torch.int32, device=dist.device)
    orow = torch.empty((nq, k), dtype=torch.int64, device=dist.device)
    _native.check((lib.emdr2_mips_merge_f32 if f32 else lib.emdr2_mips_merge)(
        dist.contiguous().data_ptr(), idx.contiguous().data_ptr(), row.contiguous().data_ptr(), s, nq, k, od.data_ptr(), oi.data_ptr(),
        orow.data_ptr(), _native.stream_ptr()), "mips_merge_f32" if f32 else "mips_merge")
    return od, oi, orow


merge_shard_results_f32 = merge_shard_results


def merge_shard_records(records, f32=False):
    """Gathered records uint8 [S, Q, k, 16] (HipIndexShard.search_records of every shard, as the all-gather delivered them) -> merged
    (dist [Q, k], idx int32, row int64): ONE launch, no casts in between."""
    lib = _native.lib()
    s, nq, k, _ = records.shape
    if records.dtype != torch.uint8 or records.shape[3] != 16 or not records.is_contiguous():
        raise ValueError("records must be a contiguous uint8 [S, Q, k, 16] tensor")
    od = torch.empty((nq, k), dtype=torch.float32 if f32 else torch.float16, device=records.device)
    oi = torch.empty((nq, k), dtype=torch.int32, device=records.device)
    orow = torch.empty((nq, k), dtype=torch.int64, device=records.device)
    _native.check(lib.emdr2_mips_merge_records(records.data_ptr(), s, nq, k, int(bool(f32)), od.data_ptr(), oi.data_ptr(), orow.data_ptr(),
                                               _native.stream_ptr()), "mips_merge_records")
    return od, oi, orow


class DistributedBruteForceIndex(object):
    """Exact inner-product top-k over the evidence embeddings (reference: emdr2_index.py:200-305).

    Same constructor and methods as the reference.  `process_group` (extra, optional) selects the
    ranks that share the index (reference: the MIPS group, mpu/initialize.py:104-142); default is
    the world group when torch.distributed is initialised, else a single shard.
    """

    def __init__(self, embed_size, embed_data=None, use_gpu=False, process_group=None, generations=False):
        self.embed_size = embed_size
        self.generations = bool(generations)                       # (extra, optional) the shard keeps generation stamps: HipIndexShard
        self._load_generation = 0                                  # the stamp of rows that add_arrays uploads: 0, or a snapshot's iteration
        self.stamps_restored = False                               # the last load_flat_snapshot set every row's own stamp from the sidecar
        self.delta_base = None                                     # {"keys", "base", "path"}: the row keys and digests of the published base snapshot (save_delta)
        self.delta_applied = None                                  # the meta of the delta the last load_flat_snapshot(delta=True) applied
        self.embed_data = embed_data
        self.use_gpu = use_gpu
        self.process_group = process_group
        self.shard = None
        self.num_rows = 0
        self.last_search_rows = None                               # global rows int64 [Q, k] of the last search_mips_index (-1 in empty slots)
        self._set_mips_index()

    # -- distributed helpers (overridable in CPU tests) ---------------------------------------------
    def _world(self):
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            return torch.distributed.get_rank(self.process_group), torch.distributed.get_world_size(self.process_group)
        return 0, 1

    def _make_shard(self, dim, n_rows, row_base):
        return HipIndexShard(dim, n_rows, row_base, generations=self.generations)

    # -- reference API -------------------------------------------------------------------------------
    def _set_mips_index(self):
        if self.embed_data is not None:
            path = getattr(self.embed_data, "embedding_path", None)
            if not self.embed_data.embed_data and path and not os.path.exists(path):
                # an empty store whose file is missing -- whether it was handed over unloaded or emptied by `update_index()`: what an eager
                # load would have said, not "rows must be float16 [N, D]" from an index over nothing
                raise FileNotFoundError("evidence embeddings not found: %s" % path)
            if not self.embed_data.embed_data and path and os.path.exists(path):
                # a store that has not been loaded (load_from_path=False): go through the flat twin of its file -- rank 0 converts, every
                # rank maps its own rows; no rank but the first ever unpickles
                self.add_flat_file(ensure_flat_embedding_file(self.embed_data.embedding_path, self.process_group))
            else:
                self.add_embed_data(self.embed_data)

    def reset_index(self):
        self.shard = None
        if self.embed_data is not None:
            embed_data_path = self.embed_data.embedding_path
            del self.embed_data
            self.embed_data = OpenRetreivalDataStore(embed_data_path, load_from_path=False)      # (loaded through its flat twin below)
            self.embed_data._lazy = True
        self._set_mips_index()

    def update_index(self):
        """emdr2_index.py:232-238: reload `embedding_path` (a new indexer job has rewritten it).  The store object stays empty: the rows
        travel pickle -> flat file (rank 0, once) -> each rank's own memory-mapped slice -> HBM."""
        self.shard = None
        if self.embed_data is not None:
            self.embed_data.clear()
        self._set_mips_index()

    # -- in-HBM refresh of this rank's rows (indexer_emdr2.IndexBuilder.build_into_index) -------------------
    def local_rows(self):
        """(first global row, one past the last) of this rank's shard; row r holds doc id `ids[r]`."""
        return self.shard.row_base, self.shard.row_base + self.shard.n_rows

    def begin_refresh(self, generation=0):
        self.shard.begin_refresh(generation)

    def refresh_rows(self, global_row, rows):
        self.shard.refresh_rows(global_row - self.shard.row_base, rows)

    def commit_refresh(self):
        self.shard.commit_refresh()

    def update_rows(self, global_row, rows, generation=None, newest_wins=False):
        """rows fp16 [n, dim] -> rows [global_row, global_row + n) of the image this rank is searching (HipIndexShard.update_rows); the
        range must lie inside this rank's shard (`local_rows()`).  `generation` / `newest_wins`: the shard's stamp rule."""
        lo, hi = self.local_rows()
        if global_row < lo or global_row + rows.shape[0] > hi:
            raise ValueError("rows [%d, %d) are not all in this rank's shard [%d, %d)" % (global_row, global_row + rows.shape[0], lo, hi))
        self.shard.update_rows(global_row - lo, rows, generation=generation, newest_wins=newest_wins)

    def update_rows_at(self, global_rows, rows, generation=None, newest_wins=False):
        """rows fp16 [n, dim], global_rows int64 [n] (both on the device) -> those rows of the image this rank is searching
        (HipIndexShard.update_rows_at).  Rows of other ranks' shards, and -1, fall out of the shard's range and are skipped: every rank can
        be handed the same gathered list.  Where a row is named twice the last occurrence wins.  `generation` / `newest_wins`: the
        shard's stamp rule, applied to the occurrence that survived."""
        self.shard.update_rows_at(global_rows - self.shard.row_base, rows, generation=generation, newest_wins=newest_wins)

    # -- generation stamps (HipIndexShard.generation_stats over every rank's shard) ------------------------------------------------------
    def generation_stats(self, now, global_rows=None):
        """Ages of the index's rows at step count `now`: of all rows, or of `global_rows` (CUDA int64, the SAME tensor on every rank, e.g.
        `last_search_rows`).  Every rank counts its own shard; the words are reduced over the index's group in at most two small
        all-reduces -- ONE sum (count, sum of ages, rows from the future, the 32 bins) and ONE max (max age and the complement of min age)
        -- issued by every rank whatever its shard holds, so the collective sequence stays static.  -> the same dict on every rank
        (`generation_result`)."""
        if self.shard is None:
            raise RuntimeError("MIPS Index is not initialized")
        mine = self.shard.generation_stats(now, global_rows)
        rank, world = self._world()
        if world == 1:
            return mine
        dist = torch.distributed
        on_device = dist.get_backend(self.process_group) == "nccl"
        place = (lambda t: t.to(self.shard.device)) if on_device else (lambda t: t)
        sums = place(torch.tensor([mine["count"], mine["sum_age"], mine["from_future"]] + mine["histogram"], dtype=torch.int64))
        # (ages are below 2^32; "no row" travels as the smallest complement, so one MAX reduces both extremes)
        none = 1 << 32
        ext = place(torch.tensor([mine["max_age"], none - min(mine["min_age"], none)], dtype=torch.int64))
        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=self.process_group)
        dist.all_reduce(ext, op=dist.ReduceOp.MAX, group=self.process_group)
        sums, ext = sums.tolist(), ext.tolist()
        min_age = _native.AUDIT_NONE if ext[1] == 0 else none - ext[1]
        return generation_result([sums[0], sums[1], min_age, ext[0], sums[2]] + sums[3:])

    def oldest_rows(self, n, below):
        """The `n` oldest rows of THIS rank's shard among those stamped below `below`, as global rows in ascending order, -1 behind them,
        and the selection's report (HipIndexShard.oldest_rows).  No collective: a rank refreshes its own rows."""
        if self.shard is None:
            raise RuntimeError("MIPS Index is not initialized")
        return self.shard.oldest_rows(n, below)

    def kept_newer(self):
        """Rows of THIS rank's shard that newest-wins updates left alone since the last call (HipIndexShard.kept_newer: one host read)."""
        return self.shard.kept_newer()

    def add_embed_data(self, all_embed_data):
        """Upload this rank's row shard (reference: emdr2_index.py:241-266; there: rank 0 uploads
        torch.chunk pieces to every visible device)."""
        ids, rows = all_embed_data.to_arrays()
        self.add_arrays(ids, rows)
        all_embed_data.clear()

    def add_flat_file(self, flat):
        """Load this rank's shard straight from a `FlatEmbeddingFile` (memory map -> pinned chunks -> HBM); only the rank's own rows are
        ever touched on the host."""
        if isinstance(flat, str):
            flat = FlatEmbeddingFile(flat)
        self.add_arrays(flat.ids, flat.rows)

    # -- audit (HipIndexShard.audit over every rank's shard) -----------------------------------------------------------------------------
    def audit(self):
        """Every rank audits its own shard; ONE int64 all_reduce(SUM) of the counters (and of how many shards use their shadow, and how
        many of those hold a non-finite row), ONE all_reduce(MIN) of the two first-offender words -> the same dict on every rank
        (`audit_result`; `first_bad_row` is a global row, `first_bad_block` the smallest offending block number local to its shard).  The
        collective sequence does not depend on what the audit finds."""
        if self.shard is None:
            raise RuntimeError("MIPS Index is not initialized")
        mine = self.shard.audit()
        rank, world = self._world()
        if world == 1:
            return mine
        dist = torch.distributed
        on_device = dist.get_backend(self.process_group) == "nccl"
        place = (lambda t: t.to(self.shard.device)) if on_device else (lambda t: t)
        bad_nf = mine["shadow_in_use"] and mine["nonfinite_rows"] > 0
        counts = place(torch.tensor([mine[n] for n in _native.AUDIT_NAMES[:12]] + [int(mine["shadow_in_use"]), int(bad_nf)], dtype=torch.int64))
        # (unsigned words through a signed reduction: 2**64 - 1, "none", travels as the largest int64)
        none = (1 << 63) - 1
        first = place(torch.tensor([min(mine[n], none) for n in ("first_bad_row", "first_bad_block")], dtype=torch.int64))
        dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=self.process_group)
        dist.all_reduce(first, op=dist.ReduceOp.MIN, group=self.process_group)
        counts, first = counts.tolist(), first.tolist()
        words = counts[:12] + [_native.AUDIT_NONE if f == none else f for f in first]
        return audit_result(words, counts[12] > 0, counts[13] > 0)

    # -- snapshots (data/index_snapshot.py) ----------------------------------------------------------------------------------------------
    def save_flat_file(self, path, meta=None, track_deltas=False):
        """Write the index as it stands in HBM to the `FlatEmbeddingFile` `path` plus `path + '.meta'` (JSON: format, n, dim, world, the
        DEVICE digest of what was exported, ids_crc32, and the caller's `meta`: iteration / refreshes / mode).  Collective and synchronous;
        the file appears atomically and a data file without a meta is an incomplete snapshot.  An index with generation stamps also
        writes every row's stamp to the sidecar `path + '.gen'` and their device digest to the meta's `stamps`.  After
        `IndexBuilder.build_into_index` this is the fast offline indexer.  `track_deltas`: also keep the key of every exported row; the
        snapshot becomes `self.delta_base`, the base of later `save_delta`s."""
        from emdr2_amd.data.index_snapshot import IndexSnapshotWriter
        writer = IndexSnapshotWriter(self, chunk_rows=min(_UPLOAD_ROWS, 1 << 18), track_deltas=track_deltas)
        writer.begin(path, meta)
        writer.finish()

    def save_delta(self, path, meta=None, max_fraction=0.5, log=None):
        """Write the rows that differ from the base snapshot at `path` -- the one `self.delta_base` describes: the last tracked
        `save_flat_file` / `IndexSnapshotWriter`, or the base a `load_flat_snapshot(delta=True)` loaded -- to `path + '.delta'` plus
        `path + '.delta.meta'` (data/index_snapshot.py).  A row is changed exactly when its key (row hash, plus stamp hash on a stamped
        index) differs from the base's, whoever wrote it; the detection pass runs on the current stream at one point in time, then ONE
        host read of its report.  Cumulative: always relative to the base, one file, replaced atomically.  Collective and synchronous.
        If any rank has more than `max_fraction` of its rows changed, or there is no base, nothing is written, a stale delta is removed
        and None is returned.  -> the delta's meta."""
        from emdr2_amd.data import index_snapshot as snap
        return snap.save_delta(self, path, meta, max_fraction, log)

    def load_flat_snapshot(self, path, audit=False, delta=False, max_iteration=None):
        """Build the index from a snapshot written by `save_flat_file` at ANY world size and verify it: meta against the file's header
        and ids, then the device digest of what now stands in HBM (combined over the ranks) against the meta's.  A mismatch raises
        ValueError.  Generation stamps, on an index that keeps them: a snapshot taken from a stamped index carries every row's stamp in
        its sidecar (`path + '.gen'`, named by the meta's `stamps`); each rank sets its own slice after its rows are in, and the device
        digest of the stamps, combined over the ranks, is checked against the meta's like the rows' -- ages after the resume are the true
        ones.  A snapshot without stamps stamps every row with the meta's `iteration` (0 if absent), and ages are then a lower bound.  An
        index without stamps ignores the sidecar.  `self.stamps_restored` says which of the two happened.
        `audit`: then run `audit()` as well (the digest covers the fp16 rows only, not emax_sq or the int8 shadow) and raise
        ValueError naming the non-zero words unless it is sound and canonical.  Returns the meta.
        `delta`: the verified base becomes `self.delta_base` (its keys are taken from the shard), so this index's own `save_delta` stays
        relative to the same base; then a delta next to the snapshot that belongs to it, and whose `iteration` is at most
        `max_iteration` (None: any), is applied and the result verified against the delta's meta (`index_snapshot.apply_delta`):
        `self.delta_applied` holds its meta.  A delta that is not this base's, is damaged or is newer than `max_iteration` is skipped --
        the base alone is a valid index -- and the returned meta says why under `"delta_skipped"`."""
        from emdr2_amd.data import index_snapshot as snap
        meta = snap.read_snapshot_meta(path)
        self.stamps_restored = False
        flat = FlatEmbeddingFile(path)
        if flat.dim != self.embed_size:
            raise ValueError("snapshot rows have %d elements, the index %d" % (flat.dim, self.embed_size))
        if snap.ids_crc32(flat.ids) != meta.get("ids_crc32"):
            raise ValueError("index snapshot %s: the doc ids do not match the meta's checksum" % path)
        self._load_generation = min(max(int(meta.get("iteration", 0) or 0), 0), _native.GEN_MAX) if self.generations else 0
        try:
            self.add_flat_file(flat)
        finally:
            self._load_generation = 0
        got = snap.index_digest(self)
        want = (int(meta["digest_sum"], 16), int(meta["digest_xor"], 16))
        if got != want:
            raise ValueError("index snapshot %s: digest %016x %016x in HBM, %016x %016x in the meta" % ((path,) + got + want))
        if self.generations and meta.get("stamps") is not None:   # (the meta and the flag are the same on every rank: so is the collective)
            lo, hi = self.local_rows()
            self.shard.set_stamps(0, snap.StampFile(snap.stamps_path(path)).stamps[lo:hi])
            got = snap.index_stamp_digest(self)
            want = (int(meta["stamps"]["digest_sum"], 16), int(meta["stamps"]["digest_xor"], 16))
            if got != want:
                raise ValueError("index snapshot %s: stamp digest %016x %016x in HBM, %016x %016x in the meta" % ((path,) + got + want))
            self.stamps_restored = True
        self.delta_applied = None
        if delta:                                                  # (what is decided below is read from files: the same on every rank)
            self.delta_base = {"keys": snap.shard_keys(self.shard), "base": snap.base_of(meta), "path": os.path.abspath(path)}
            try:
                dmeta = snap.read_delta_meta(path, meta)
                if max_iteration is not None and int(dmeta["iteration"]) > int(max_iteration):
                    meta["delta_skipped"] = "the delta is of iteration %d, beyond %d" % (int(dmeta["iteration"]), int(max_iteration))
                    dmeta = None
            except FileNotFoundError:
                dmeta = None
            except ValueError as exc:
                meta["delta_skipped"], dmeta = str(exc), None
            if dmeta is not None:
                snap.apply_delta(self, path, dmeta)
                self.delta_applied = dmeta
        if audit:
            bad = audit_failures(self.audit())
            if bad:
                raise ValueError("index snapshot %s: the index audit failed: %s" % (path, bad))
        return meta

    def add_arrays(self, ids, rows):
        if rows.dtype != np.float16 or rows.shape[1] != self.embed_size:
            raise ValueError("rows must be float16 [N, %d]" % self.embed_size)
        self.num_rows = rows.shape[0]
        rank, world = self._world()
        lo, hi = shard_bounds(self.num_rows, world)[rank]
        self.shard = self._make_shard(self.embed_size, hi - lo, lo)
        if hi > lo:
            if getattr(self.shard, "generation", None) is not None:
                self.shard.append_rows(rows[lo:hi], generation=self._load_generation)
            else:
                self.shard.append_rows(rows[lo:hi])
            self.shard.set_ids(ids[lo:hi])

    def search_mips_index(self, query_embeds, top_k, reconstruct=True):
        """(distances fp16 [Q,k], indices int32 [Q,k]) on the device, indices are doc ids
        (reference: emdr2_index.py:268-305; `reconstruct` is ignored there too).  Every rank passes the
        same all-gathered query block (emdr2_model.py:438-444) and receives the same result."""
        if self.shard is None:
            raise RuntimeError("MIPS Index is not initialized")
        q = query_embeds
        if q.dtype != torch.float16:
            q = q.to(torch.float16)   # reference queries are fp16 under FP16_Module; bf16/fp32 are rounded once
        rank, world = self._world()
        if world == 1:
            dist, idx, self.last_search_rows, _ = self.shard.search(q.contiguous(), top_k)
            return dist, idx
        dist, idx, self.last_search_rows = self._search_exchange_merge(q.contiguous(), top_k, rank, world, f32=False)
        return dist, idx

    def _search_exchange_merge(self, q, top_k, rank, world, f32):
        """Sharded search: the shard scan's last kernel writes its packed records straight into this rank's slice of the gather buffer, ONE
        all-gather (16 bytes per (query, slot) and rank: 410 KB at 512 x 50), ONE merge launch on the gathered buffer.  Nothing else runs
        between them; `exchange_events` (when a list) receives a (start, end) event pair around all-gather + merge."""
        nq = q.shape[0]
        gathered = torch.empty((world, nq, top_k, 16), dtype=torch.uint8, device=q.device)
        self.shard.search_records(q, top_k, f32=f32, out=gathered[rank])
        ev = getattr(self, "exchange_events", None)
        if ev is not None and len(ev) < 4096:
            pair = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            pair[0].record()
        else:
            pair = None
        self._all_gather_records(gathered, rank)
        out = self._merge_records(gathered, f32)
        if pair is not None:
            pair[1].record()
            ev.append(pair)
        return out

    def _all_gather_records(self, gathered, rank):
        # RCCL: in place -- this rank's slice of `gathered` (which its finalize kernel has just written) IS its send buffer (the in-place
        # form of ncclAllGather: sendbuff == recvbuff + rank * count).  Other transports (gloo in the dry runs) get a private copy.
        mine = gathered[rank]
        if torch.distributed.get_backend(self.process_group) != "nccl":
            mine = mine.clone()
        # (output = the ranks' inputs concatenated along dim 0: gloo checks the shapes, RCCL only the element count)
        torch.distributed.all_gather_into_tensor(gathered.view((-1,) + tuple(gathered.shape[2:])), mine, group=self.process_group)

    def _merge_records(self, gathered, f32):
        return merge_shard_records(gathered, f32)

    # -- stored vectors by global row (search_and_reconstruct; --context-embeddings-from-index) ------------------------------------------
    def reconstruct_rows(self, global_rows, scatter=False):
        """The stored fp16 vectors of `global_rows` (CUDA int64 [...], as a search returns them: `last_search_rows`) -> CUDA fp16
        [..., dim], bit for bit, at any world size; -1 (an empty slot) gives a zero vector.  Collective when the index is sharded: every
        rank passes the SAME row tensor and every rank receives all vectors.  Each rank gathers its own rows into a buffer whose foreign
        rows are zero (HipIndexShard.rows_global); the buffer, viewed as int32 (RCCL has no 16-bit integer type), goes through ONE
        all_reduce(SUM): exactly one rank contributes non-zero bits to a row, so the integer sum hands back the stored bits -- -0.0, inf
        and NaN payloads included, which a floating-point sum would not.  `scatter`: return only this rank's slice of the leading
        dimension (which the world size must divide): reduce_scatter_tensor on RCCL, all_reduce + slice on other transports.  Enqueued on
        the current stream, in the same order against in-place updates as a search: the caller orders it."""
        if self.shard is None:
            raise RuntimeError("MIPS Index is not initialized")
        rank, world = self._world()
        if world == 1:
            return self.shard.rows_global(global_rows)
        n = global_rows.shape[0] if global_rows.dim() else 0
        if scatter and (global_rows.dim() < 1 or n % world):
            raise ValueError("scatter: the world size %d must divide the leading dimension of %s" % (world, tuple(global_rows.shape)))
        buf = self.shard.rows_global(global_rows)
        if buf.numel() == 0:
            return buf[rank * (n // world):(rank + 1) * (n // world)] if scatter else buf
        words = buf.view(torch.int32)                                # (dim % 32 == 0: whole words)
        if scatter and torch.distributed.get_backend(self.process_group) == "nccl":
            mine = torch.empty((n // world,) + tuple(buf.shape[1:]), dtype=torch.float16, device=buf.device)
            torch.distributed.reduce_scatter_tensor(mine.view(torch.int32), words, op=torch.distributed.ReduceOp.SUM, group=self.process_group)
            return mine
        torch.distributed.all_reduce(words, op=torch.distributed.ReduceOp.SUM, group=self.process_group)
        return buf[rank * (n // world):(rank + 1) * (n // world)] if scatter else buf


class FaissMIPSIndex(DistributedBruteForceIndex):
    """The evaluator's index (reference: emdr2_index.py:103-197: `faiss.IndexFlatIP(embed_size)` under `IndexIDMap`, optionally
    `index_cpu_to_all_gpus(shard=True, useFloat16=True)`; callers: tasks/openqa/dense_retriever/evaluation/evaluate.py:49,123).
    Same constructor and methods; `search_mips_index` returns numpy `(distances float32 [Q,k], indices int64 [Q,k])` like faiss, or with
    `reconstruct=True` the `search_and_reconstruct` triple `(distances, indices, vectors float32 [Q,k,dim])`.

    MI355X-native: the same row-sharded stripe-tiled fp16 image and scan as the training index (faiss's useFloat16 storage), scores
    = RNE_fp32(exact dot) with order (score desc, row asc) -- the exact-arithmetic restatement of IndexFlatIP (oracle: topk_f32).  Vectors
    are stored in fp16 (`add_block_data` already produced fp16, emdr2_index.py:61); queries are rounded to fp16 once (the evaluator's
    queries come out of the fp16 model, so `np.float32(query)` there holds fp16 values).  faiss is absent from /root/reference and
    unpinned: parity against faiss itself is unpinned; against the oracle it is bit-exact."""

    def add_with_ids(self, embeds, ids):
        """faiss `IndexIDMap.add_with_ids` (emdr2_index.py:177): float32 / float16 rows keyed by int64 ids."""
        rows = np.ascontiguousarray(np.asarray(embeds), dtype=np.float16)
        self.add_arrays(np.asarray(ids), rows)

    def search_mips_index(self, query_embeds, top_k, reconstruct=True):
        if self.shard is None:
            raise RuntimeError("MIPS Index is not initialized")
        q = torch.as_tensor(query_embeds)
        q = q.to(device=self.shard.device, dtype=torch.float16).contiguous()
        rank, world = self._world()
        if world > 1:
            dist, idx, row = self._search_exchange_merge(q, top_k, rank, world, f32=True)
        else:
            dist, idx, row, _ = self.shard.search_f32(q, top_k)
        distances = dist.cpu().numpy()
        indices = idx.to(torch.int64).cpu().numpy()
        if not reconstruct:
            return distances, indices
        # the hit vectors by their merged global rows, wherever they live (one all-reduce when sharded); an empty slot (row -1) is a zero vector
        vecs = self.reconstruct_rows(row.contiguous()).to(torch.float32)
        return distances, indices, vecs.cpu().numpy()
