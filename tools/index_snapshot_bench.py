"""Index snapshots, measured: the two kernels, a synchronous save and load, and what the paced writer costs a training step.

1. kernels   `emdr2_mips_export_rows` and `emdr2_mips_digest_rows` over a whole shard of N/8 = 2,626,916 x 768 rows and over the full
             21,015,324 rows, next to a device-to-device copy of the same bytes timed the same way (device events, 2 warm-ups, `--calls`
             timed calls, alternating).  GB/s counts the bytes a call moves: read + written for the export and the copy, read for the digest.
2. save/load wall time of `save_flat_file` and `load_flat_snapshot` of the N/8 shard (files under --dir), and their parts measured alone:
             export + device-to-host copies, the file write of the same bytes, the digest, the ids checksum.
3. step      the `e2e_k100` step of bench.py (bench_e2e.setup at its per-rank shape, side-stream refresher at the 8-GPU pace) WITHOUT and
             WITH a paced snapshot (`IndexSnapshotWriter.pump` + `maybe_finalize` at every step boundary, chunk = the default pace of a
             500-step reload interval), alternating blocks of steps in one process.  Without the writer the step runs no snapshot code: it is
             the parent's step.
4. stamps    (only when asked for) generation stamps in snapshots: `emdr2_mips_digest_stamps` over the 2,626,916 stamps of an N/8 shard next
             to `emdr2_mips_generation_stats` and a copy of the same words, and one pump at the N/8 shard's paced chunk on a shard without
             and with stamps, alternating (`--what stamps --out profiles/index_snapshot_stamps.txt`).
usage: python tools/index_snapshot_bench.py [--what kernels save step] [--calls 10] [--out profiles/index_snapshot.txt]"""
import argparse
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
import bench_e2e  # noqa: E402
from emdr2_amd import _native  # noqa: E402
from emdr2_amd.data import index_snapshot as snap  # noqa: E402
from emdr2_amd.data.emdr2_index import FlatEmbeddingFile, HipIndexShard  # noqa: E402

DIM, WARMUP = 768, 2
SHARD_ROWS, FULL_ROWS = 2626916, 21015324


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


def rate_line(name, ms, nbytes):
    med = statistics.median(ms)
    return "  %-44s median %8.3f ms  min %8.3f  max %8.3f  (%d calls)  %8.1f GB/s at the median" % (name, med, min(ms), max(ms), len(ms), nbytes / med / 1e6)


def kernels(n_rows, calls):
    sh = HipIndexShard(DIM, n_rows, 0, shadow=False)
    for blk in bench.synth_rows(0, n_rows):
        sh.append_rows(blk)
    nbytes = n_rows * DIM * 2
    out = torch.empty((n_rows, DIM), dtype=torch.float16, device="cuda")
    acc = torch.zeros(2, dtype=torch.int64, device="cuda")
    flat = out.view(torch.uint8).reshape(-1)
    fns = (("export", lambda: sh.export_rows(0, n_rows, out=out)), ("digest", lambda: sh.digest_into(acc, 0, n_rows)),
           ("copy", lambda: flat.copy_(sh.tiled[:nbytes])))
    t = {name: [] for name, _ in fns}
    for i in range(WARMUP + calls):
        for name, fn in fns:
            ms = timed_ms(fn)
            if i >= WARMUP:
                t[name].append(ms)
    lines = ["%d rows x %d fp16 (%.2f GB image)" % (n_rows, DIM, nbytes / 1e9),
             rate_line("emdr2_mips_export_rows (read + written)", t["export"], 2 * nbytes),
             rate_line("emdr2_mips_digest_rows (read)", t["digest"], nbytes),
             rate_line("device-to-device copy (read + written)", t["copy"], 2 * nbytes)]
    read_rate_of_copy = nbytes / statistics.median(t["copy"]) / 1e6
    digest_rate = nbytes / statistics.median(t["digest"]) / 1e6
    bound = "VALU" if digest_rate < 0.8 * read_rate_of_copy else "HBM"
    lines.append("  digest reads %.1f GB/s where the copy reads %.1f GB/s (and writes as much): the digest is %s-bound "
                 "(two 64-bit multiplies per 4 bytes; below 0.8 x the copy's read rate counts as VALU)" % (digest_rate, read_rate_of_copy, bound))
    return lines


def save_and_load(dir_):
    index = bench_e2e.build_index(SHARD_ROWS, 0, 1)
    shard = index.shard
    nbytes = SHARD_ROWS * DIM * 2
    path = os.path.join(dir_, "index_snapshot_bench.flat")
    lines = ["synchronous save / load of %d rows x %d (%.2f GB of rows), files under %s" % (SHARD_ROWS, DIM, nbytes / 1e9, dir_)]
    try:
        for rep in range(2):
            s, _ = wall_s(lambda: index.save_flat_file(path, {"mode": "build"}))
            lines.append("  save_flat_file, run %d                          %8.2f s  (%.2f GB/s)" % (rep + 1, s, nbytes / s / 1e9))
        # the parts, alone: export + D2H through the writer's two pinned buffers without a file; the digest; the file write of the same bytes
        chunk = snap.SNAPSHOT_ROWS
        dev = torch.empty((chunk, DIM), dtype=torch.float16, device="cuda")
        pinned = [torch.empty((chunk, DIM), dtype=torch.float16).pin_memory() for _ in range(2)]

        def d2h():
            for i, lo in enumerate(range(0, SHARD_ROWS, chunk)):
                m = min(chunk, SHARD_ROWS - lo)
                shard.export_rows(lo, m, out=dev)
                pinned[i & 1][:m].copy_(dev[:m], non_blocking=True)
        s, _ = wall_s(d2h)
        lines.append("    export + device-to-host copies alone          %8.2f s  (%.2f GB/s)" % (s, nbytes / s / 1e9))
        s, _ = wall_s(lambda: shard.digest())
        lines.append("    device digest of the shard (one readback)     %8.4f s" % s)

        def file_write():
            f = FlatEmbeddingFile.create(path + ".w", SHARD_ROWS, DIM)
            host = pinned[0].numpy()
            for lo in range(0, SHARD_ROWS, chunk):
                m = min(chunk, SHARD_ROWS - lo)
                f.rows[lo:lo + m] = host[:m]
            f.flush()
        s, _ = wall_s(file_write)
        os.remove(path + ".w")
        lines.append("    file write of the same bytes alone (memory map + flush) %6.2f s  (%.2f GB/s)" % (s, nbytes / s / 1e9))
        for rep in range(2):
            fresh = type(index)(embed_size=DIM, embed_data=None, use_gpu=True)
            s, _ = wall_s(lambda: fresh.load_flat_snapshot(path))
            lines.append("  load_flat_snapshot incl. the digest check, run %d %8.2f s  (%.2f GB/s)" % (rep + 1, s, nbytes / s / 1e9))
            del fresh
        fresh = type(index)(embed_size=DIM, embed_data=None, use_gpu=True)
        s, _ = wall_s(lambda: fresh.add_flat_file(path))
        lines.append("    add_flat_file alone (file -> pinned -> HBM, pack, seal) %6.2f s" % s)
        s, _ = wall_s(lambda: snap.index_digest(fresh))
        lines.append("    device digest + combine                       %8.4f s" % s)
        s, _ = wall_s(lambda: snap.ids_crc32(FlatEmbeddingFile(path).ids))
        lines.append("    ids checksum                                  %8.4f s" % s)
    finally:
        for p in (path, snap.meta_path(path), path + ".w"):
            if os.path.exists(p):
                os.remove(p)
    return lines


def step_cost(dir_, blocks, steps):
    ap = argparse.ArgumentParser()
    bench_e2e.add_args(ap)
    a = ap.parse_args([])
    from emdr2_amd.tasks.openqa.e2eqa.async_indexer import PACE_MARGIN
    interval, ranks = 500, 8
    a.rows, a.micro_batches = SHARD_ROWS, 8
    a.reindex_rows_per_step = (FULL_ROWS + ranks * int(interval * PACE_MARGIN) - 1) // (ranks * int(interval * PACE_MARGIN))
    index = bench_e2e.build_index(SHARD_ROWS, 0, 1)
    ctx = bench_e2e.setup(a, 0, 1, index=index, topk=100)
    chunk = snap.IndexSnapshotWriter.paced_chunk_rows(SHARD_ROWS, interval)
    writer = snap.IndexSnapshotWriter(index, chunk_rows=chunk)
    path = os.path.join(dir_, "index_snapshot_bench_step.flat")
    it = [0]

    def block(with_writer):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            ctx.step()
            it[0] += 1
            if with_writer:
                writer.pump()
                writer.maybe_finalize(it[0])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps
    lines = ["e2e_k100 step (B=%d, top-k 100, %d-row shard, refresher at %d rows per step) without / with the paced snapshot: %d rows (%.1f MB) "
             "exported per step" % (a.batch, SHARD_ROWS, a.reindex_rows_per_step, chunk, chunk * DIM * 2 / 1e6)]
    try:
        for _ in range(2):
            ctx.step()
        writer.begin(path, {"iteration": 0, "refreshes": 0, "mode": "swap"})
        t = {False: [], True: []}
        for _ in range(blocks):
            for with_writer in (False, True):
                t[with_writer].append(block(with_writer))
        pumped = writer._cursor
        s, _ = wall_s(writer.finish)
        for with_writer in (False, True):
            lines.append("  %-10s ms per step, %d blocks of %d steps: %s   median %.1f" % (
                "with" if with_writer else "without", blocks, steps, " ".join("%.1f" % v for v in t[with_writer]), statistics.median(t[with_writer])))
        wo, w = statistics.median(t[False]), statistics.median(t[True])
        lines.append("  per-step cost of the paced snapshot: %+.1f ms = %+.2f %% of the step (run-to-run spread of this pool: 3 %%)" % (w - wo, (w / wo - 1) * 100))
        lines.append("  %d of %d rows were exported by the pumps; the blocking finish() of the rest took %.2f s" % (pumped, SHARD_ROWS, s))
    finally:
        for p in (path, snap.meta_path(path)):
            if os.path.exists(p):
                os.remove(p)
    return lines


def stamps(dir_, calls, parent_module=None):
    """Generation stamps in snapshots: the stamp digest over an N/8 shard's stamps next to `generation_stats` and a copy of the same words;
    one pump at the N/8 shard's paced chunk on a shard without and with stamps, alternating (without stamps a pump makes exactly the calls
    it made before there were stamps in snapshots).  `parent_module`: a copy of the PARENT commit's emdr2_amd/data/index_snapshot.py
    (`git show HEAD~1:emdr2_amd/data/index_snapshot.py > FILE`); its writer pumps a third shard, without stamps, in the same alternation."""
    import importlib.util
    from emdr2_amd.data.emdr2_index import DistributedBruteForceIndex
    arms = [("this commit, shard without stamps", snap, False), ("this commit, shard with stamps", snap, True)]
    if parent_module:
        spec = importlib.util.spec_from_file_location("parent_index_snapshot", parent_module)
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
        arms.insert(0, ("the parent commit's writer, shard without stamps", parent, False))
    lib = _native.lib()
    gen = torch.randint(0, 1 << 31, (SHARD_ROWS,), dtype=torch.int64, device="cuda").to(torch.int32)
    twin = torch.empty_like(gen)
    acc = torch.zeros(2, dtype=torch.int64, device="cuda")
    report = torch.empty(_native.GEN_WORDS, dtype=torch.int64, device="cuda")
    stream = _native.stream_ptr()
    fns = (("digest", lambda: _native.check(lib.emdr2_mips_digest_stamps(gen.data_ptr(), SHARD_ROWS, 0, SHARD_ROWS, 0, acc.data_ptr(), stream), "digest_stamps")),
           ("digest+1", lambda: _native.check(lib.emdr2_mips_digest_stamps(gen.data_ptr(), SHARD_ROWS, 1, SHARD_ROWS - 2, 0, acc.data_ptr(), stream), "digest_stamps")),
           ("stats", lambda: _native.check(lib.emdr2_mips_generation_stats(gen.data_ptr(), SHARD_ROWS, 0, None, 0, 1 << 31, report.data_ptr(), stream), "generation_stats")),
           ("copy", lambda: twin.copy_(gen)))
    t = {name: [] for name, _ in fns}
    for i in range(WARMUP + 2 * calls):
        for name, fn in fns:
            ms = timed_ms(fn)
            if i >= WARMUP:
                t[name].append(ms * 1e3)
    us = lambda name, v: "  %-58s median %8.1f us  min %8.1f  max %8.1f  (%d calls)" % (name, statistics.median(v), min(v), max(v), len(v))
    lines = ["%d stamps (%.1f MB), device events around one call" % (SHARD_ROWS, SHARD_ROWS * 4 / 1e6),
             us("emdr2_mips_digest_stamps, the whole shard", t["digest"]),
             us("emdr2_mips_digest_stamps, rows 1 .. n - 2 (scalar head and tail)", t["digest+1"]),
             us("emdr2_mips_generation_stats, the whole shard", t["stats"]),
             us("device-to-device copy of the stamps", t["copy"])]
    # one pump: a shard of 40 paced chunks, 768 wide (the chunk, not the shard's length, sets a pump's work)
    chunk = snap.IndexSnapshotWriter.paced_chunk_rows(SHARD_ROWS, 500)
    n_rows = 40 * chunk
    writers, paths = [], []
    for k, (_, mod, stamped) in enumerate(arms):
        index = DistributedBruteForceIndex(DIM, None, use_gpu=True, generations=stamped)
        sh = HipIndexShard(DIM, n_rows, 0, shadow=False, generations=stamped)
        for blk in bench.synth_rows(0, n_rows):
            sh.append_rows(blk)
        if stamped:
            sh.generation.copy_(gen[:n_rows])
        index.shard, index.num_rows = sh, n_rows
        writers.append(mod.IndexSnapshotWriter(index, chunk_rows=chunk))
        paths.append(os.path.join(dir_, "index_snapshot_bench_stamps%d.flat" % k))
        writers[-1].begin(paths[-1], {"mode": "rolling"})
    dev, host = [[] for _ in arms], [[] for _ in arms]
    try:
        for i in range(WARMUP + min(calls, 30)):
            for k, writer in enumerate(writers):
                torch.cuda.synchronize()                         # (both buffers free again: the pump below exports)
                while writer._free.qsize() < 2:
                    time.sleep(0.001)
                before = writer._cursor
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                t0 = time.perf_counter()
                writer.pump()
                wall = (time.perf_counter() - t0) * 1e3
                b.record()
                b.synchronize()
                ms = a.elapsed_time(b)
                assert writer._cursor == before + chunk
                if i >= WARMUP:
                    dev[k].append(ms * 1e3); host[k].append(wall * 1e3)
        lines.append("one pump of %d rows x %d (%.1f MB of rows, %.1f KB of stamps), alternating; device events around pump() on the step's stream "
                     "(the device-to-host copies run on the side stream behind it), and the host's wall time of the call, which only enqueues"
                     % (chunk, DIM, chunk * DIM * 2 / 1e6, chunk * 4 / 1e3))
        for k, (name, _, _) in enumerate(arms):
            lines.append(us("%s, on the stream" % name, dev[k]))
            lines.append(us("%s, host time of the call" % name, host[k]))
        lines.append("  with - without stamps on this commit, medians: %+.1f us on the stream, %+.1f us of host time"
                     % (statistics.median(dev[-1]) - statistics.median(dev[-2]), statistics.median(host[-1]) - statistics.median(host[-2])))
    finally:
        for writer in writers:
            writer.finish()
        for p in paths:
            for q in (p, snap.meta_path(p), snap.stamps_path(p)):
                if os.path.exists(q):
                    os.remove(q)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", nargs="+", default=["kernels", "save", "step"], choices=["kernels", "save", "step", "stamps"])
    ap.add_argument("--rows", type=int, nargs="+", default=[SHARD_ROWS, FULL_ROWS])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--dir", default=tempfile.gettempdir())
    ap.add_argument("--parent-module", default=None, help="--what stamps: a copy of the parent commit's emdr2_amd/data/index_snapshot.py")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_snapshot.txt"))
    args = ap.parse_args()
    with open(_native.LIB_PATH, "rb") as fh:
        sha = hashlib.sha256(fh.read()).hexdigest()
    text = ["index snapshots (tools/index_snapshot_bench.py); device: %s; libemdr2_hip.so sha256 %s" % (torch.cuda.get_device_name(0), sha)]

    def emit(lines):
        text.extend([""] + lines)
        print("\n".join(lines), flush=True)
    if "kernels" in args.what:
        for n in args.rows:
            emit(kernels(n, args.calls))
            torch.cuda.empty_cache()
    if "save" in args.what:
        emit(save_and_load(args.dir))
        torch.cuda.empty_cache()
    if "step" in args.what:
        emit(step_cost(args.dir, args.blocks, args.steps))
    if "stamps" in args.what:
        emit(stamps(args.dir, args.calls, args.parent_module))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
