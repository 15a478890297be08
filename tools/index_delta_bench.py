"""Incremental index snapshots, measured: the detection pass next to the digest pass it is modelled on, and a delta's save and load.

1. kernels   `HipIndexShard.changed_rows` over a shard of N/8 = 2,626,916 x 768 rows and over the full 21,015,324 rows with 0 %, 1 %, 10 %
             and 100 % of the rows changed (cap = the shard's rows), next to `emdr2_mips_digest_rows` over the same shard -- this commit's
             and, with `--parent-module`, the PARENT commit's library (a libemdr2_hip.so built from it) -- and a device-to-device copy of
             the same bytes.  Device events around one call, 2 warm-ups, `--calls` timed calls, the arms alternating, medians.
2. save/load wall time of `save_delta` and of `load_flat_snapshot(delta=True)` on the N/8 shard at 1 % and 10 % changed rows (files under
             --dir), split into their parts: detection + its one host read, the gather of the changed rows, the copies to the host and
             the file; the base load, the keys, reading and applying the delta, the digest checks.  Disk and pinned-copy times are
             recorded, not judged.
usage: python tools/index_delta_bench.py [--what kernels save] [--rows N ...] [--calls 10] [--parent-module PARENT/libemdr2_hip.so]
                                         [--out profiles/index_delta.txt]"""
import argparse
import ctypes
import hashlib
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from emdr2_amd import _native  # noqa: E402
from emdr2_amd.data import index_snapshot as snap  # noqa: E402
from emdr2_amd.data.emdr2_index import DistributedBruteForceIndex, HipIndexShard  # noqa: E402

DIM, WARMUP = 768, 2
SHARD_ROWS, FULL_ROWS = 2626916, 21015324
FRACTIONS = (0.0, 0.01, 0.1, 1.0)


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def wall_s(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def line(name, ms, nbytes=None):
    med = statistics.median(ms)
    rate = "" if nbytes is None else "  %8.1f GB/s read at the median" % (nbytes / med / 1e6)
    return "  %-58s median %8.3f ms  min %8.3f  max %8.3f  (%d calls)%s" % (name, med, min(ms), max(ms), len(ms), rate)


def filled_shard(n_rows, generations=True):
    sh = HipIndexShard(DIM, n_rows, 0, shadow=False, generations=generations)
    for blk in bench.synth_rows(0, n_rows):
        sh.append_rows(blk)
    return sh


def damaged_keys(keys, fraction, seed=1):
    """a copy of `keys` with about `fraction` of the entries flipped: those rows report as changed (the pass only compares)"""
    out = keys.clone()
    if fraction >= 1.0:
        out ^= 1
    elif fraction > 0.0:
        g = torch.Generator(device=keys.device).manual_seed(seed)
        hit = torch.rand(keys.numel(), device=keys.device, generator=g) < fraction
        out[hit] ^= 1
    return out


def kernels(n_rows, calls, parent_lib):
    sh = filled_shard(n_rows)
    nbytes = n_rows * DIM * 2
    keys = sh.row_keys()
    acc = torch.zeros(2, dtype=torch.int64, device="cuda")
    twin = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = _native.stream_ptr()
    fns = []
    counts = {}
    for f in FRACTIONS:
        base = damaged_keys(keys, f)
        name = "changed_rows, %g %% changed" % (100 * f)
        fns.append((name, lambda base=base: sh.changed_rows(base, n_rows)))
        counts[name] = int(sh.changed_rows(base, 0)[1][0].item())
    fns.append(("digest", lambda: sh.digest_into(acc, 0, n_rows)))
    if parent_lib is not None:
        parent_digest = parent_lib.emdr2_mips_digest_rows
        parent_digest.restype, parent_digest.argtypes = _native.SIGNATURES["emdr2_mips_digest_rows"]
        fns.append(("parent digest", lambda: _native.check(parent_digest(sh.tiled.data_ptr(), n_rows, DIM, 0, n_rows, 0, acc.data_ptr(), stream),
                                                           "parent digest_rows")))
    fns.append(("copy", lambda: twin.copy_(sh.tiled[:nbytes])))
    t = {name: [] for name, _ in fns}
    for i in range(WARMUP + calls):
        for name, fn in fns:
            ms = timed_ms(fn)
            if i >= WARMUP:
                t[name].append(ms)
    out = ["%d rows x %d fp16 (%.2f GB image, %.1f MB of keys, %.1f MB of stamps), device events around one call"
           % (n_rows, DIM, nbytes / 1e9, n_rows * 8 / 1e6, n_rows * 4 / 1e6)]
    for f in FRACTIONS:
        name = "changed_rows, %g %% changed" % (100 * f)
        out.append(line("%s (%d rows reported)" % (name, counts[name]), t[name], nbytes + 12 * n_rows))
    out.append(line("emdr2_mips_digest_rows, this commit", t["digest"], nbytes))
    if parent_lib is not None:
        out.append(line("emdr2_mips_digest_rows, the parent commit's library", t["parent digest"], nbytes))
    out.append(line("device-to-device copy of the image (read + written)", t["copy"], nbytes))
    ref = t["parent digest"] if parent_lib is not None else t["digest"]
    extra = statistics.median(t["changed_rows, 0 % changed"]) - statistics.median(ref)
    out.append("  changed_rows at 0 %% - the %s digest pass, medians: %+.1f us (the digest arm's own spread: %.1f us)"
               % ("parent's" if parent_lib is not None else "commit's own", extra * 1e3, (max(ref) - min(ref)) * 1e3))
    return out


def save_and_load(dir_, fractions=(0.01, 0.1)):
    index = DistributedBruteForceIndex(DIM, None, use_gpu=True, generations=True)
    index.shard, index.num_rows = filled_shard(SHARD_ROWS), SHARD_ROWS
    index.shard.set_ids(torch.arange(1, SHARD_ROWS + 1, dtype=torch.int32).numpy())
    sh = index.shard
    path = os.path.join(dir_, "index_delta_bench.flat")
    out = ["save_delta / load with a delta, %d rows x %d, files under %s" % (SHARD_ROWS, DIM, dir_)]
    try:
        s, _ = wall_s(lambda: index.save_flat_file(path, {"iteration": 1}, track_deltas=True))
        out.append("  save_flat_file(track_deltas=True), the base                 %8.2f s" % s)
        generation = 2
        for f in fractions:
            k = int(SHARD_ROWS * f) - int(SHARD_ROWS * (fractions[0] if f != fractions[0] else 0))     # cumulative: up to f in all
            g = torch.Generator(device="cuda").manual_seed(generation)
            ids = torch.randperm(SHARD_ROWS, device="cuda", generator=g)[:k].contiguous()
            for lo in range(0, k, 1 << 16):
                part = ids[lo:lo + (1 << 16)]
                rows = torch.randn((part.numel(), DIM), device="cuda", generator=g).half()
                index.update_rows_at(part, rows, generation=generation)
            generation += 1
            cap = SHARD_ROWS // 2
            s_detect, (rows, info) = wall_s(lambda: (lambda r, i: (r, i.tolist()))(*sh.changed_rows(index.delta_base["keys"], cap)))
            m = info[1]
            s_gather, data = wall_s(lambda: (sh.rows_global(rows[:m]), sh.generation[rows[:m]]))
            pinned = torch.empty((min(m, snap.DELTA_ROWS), DIM), dtype=torch.float16).pin_memory()

            def to_host():
                for lo in range(0, m, snap.DELTA_ROWS):
                    pinned[:min(snap.DELTA_ROWS, m - lo)].copy_(data[0][lo:lo + snap.DELTA_ROWS])
            s_host, _ = wall_s(to_host)
            s_save, meta = wall_s(lambda: index.save_delta(path, {"iteration": generation}))
            size = os.path.getsize(snap.delta_path(path))
            out.append("  %g %% changed: %d rows, a delta of %.1f MB" % (100 * f, meta["m"], size / 1e6))
            out.append("    save_delta                                               %8.3f s" % s_save)
            out.append("      detection pass + the one host read alone               %8.4f s" % s_detect)
            out.append("      gather of the changed rows and stamps alone            %8.4f s" % s_gather)
            out.append("      copies to the host through one pinned buffer alone     %8.4f s" % s_host)
            out.append("      the rest (file, flush, checksum, meta, renames)        %8.3f s" % (s_save - s_detect - s_gather - s_host))
            fresh = DistributedBruteForceIndex(DIM, None, use_gpu=True, generations=True)
            s_load, _ = wall_s(lambda: fresh.load_flat_snapshot(path, delta=True))
            assert fresh.delta_applied == meta
            alone = DistributedBruteForceIndex(DIM, None, use_gpu=True, generations=True)
            s_base, _ = wall_s(lambda: alone.load_flat_snapshot(path))
            s_keys, _ = wall_s(lambda: alone.shard.row_keys())
            s_meta, dmeta = wall_s(lambda: snap.read_delta_meta(path))
            s_apply, _ = wall_s(lambda: snap.apply_delta(alone, path, dmeta))
            out.append("    load_flat_snapshot(delta=True)                           %8.3f s" % s_load)
            out.append("      the base alone (load_flat_snapshot)                    %8.3f s" % s_base)
            out.append("      row_keys over the shard                                %8.4f s" % s_keys)
            out.append("      read_delta_meta (header, checksum of the row list)     %8.4f s" % s_meta)
            out.append("      apply_delta (file -> HBM, update_rows_at, stamps, both digest checks) %8.3f s" % s_apply)
            del fresh, alone
            torch.cuda.empty_cache()
    finally:
        for p in (path, snap.meta_path(path), snap.stamps_path(path), snap.delta_path(path), snap.delta_meta_path(path)):
            if os.path.exists(p):
                os.remove(p)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["kernels", "save"], choices=["kernels", "save"])
    ap.add_argument("--rows", type=int, nargs="+", default=[SHARD_ROWS, FULL_ROWS])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--parent-module", default=None, help="a libemdr2_hip.so built from the parent commit: its emdr2_mips_digest_rows is timed in the same alternation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_delta.txt"))
    args = ap.parse_args()
    with open(_native.LIB_PATH, "rb") as fh:
        sha = hashlib.sha256(fh.read()).hexdigest()
    text = ["incremental index snapshots (tools/index_delta_bench.py); device: %s; libemdr2_hip.so sha256 %s" % (torch.cuda.get_device_name(0), sha)]
    parent_lib = None
    if args.parent_module:
        parent_lib = ctypes.CDLL(args.parent_module)
        with open(args.parent_module, "rb") as fh:
            text.append("the parent commit's library: sha256 %s" % hashlib.sha256(fh.read()).hexdigest())

    def emit(lines):
        text.extend([""] + lines)
        print("\n".join(lines), flush=True)
    if "kernels" in args.what:
        for n in args.rows:
            emit(kernels(n, args.calls, parent_lib))
            torch.cuda.empty_cache()
    if "save" in args.what:
        emit(save_and_load(args.dir))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
