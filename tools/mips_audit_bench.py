"""The index audit, measured: device-event time of one `emdr2_mips_audit` over a shard of N/8 = 2,626,916 x 768 rows and over the full
21,015,324 rows, without and with the int8 shadow image (block-norm table passed in both), next to a device-to-device copy of the bytes
the audit reads, timed the same way (2 warm-ups, `--calls` timed calls, alternating) -- the yardstick of tools/index_snapshot_bench.py.
GB/s counts the bytes the audit reads from HBM once: the fp16 image, plus the int8 image with a shadow (its re-reads of a 256-row block
come out of L2); the copy reads the same bytes and writes as many.  The audit's one host read of 128 bytes is not in the device time;
`HipIndexShard.audit()` (enqueue + read-back, wall clock) is given next to it.  No threshold: the numbers are recorded.
usage: python tools/mips_audit_bench.py [--rows 2626916 21015324] [--calls 10] [--out profiles/mips_audit.txt]"""
import argparse
import ctypes
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from emdr2_amd import _native  # noqa: E402
from emdr2_amd.data.emdr2_index import HipIndexShard  # noqa: E402

DIM, WARMUP = 768, 2
SHARD_ROWS, FULL_ROWS = 2626916, 21015324


def timed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def rate_line(name, ms, nbytes):
    med = statistics.median(ms)
    return "  %-52s median %8.3f ms  min %8.3f  max %8.3f  (%d calls)  %8.1f GB/s at the median" % (name, med, min(ms), max(ms), len(ms), nbytes / med / 1e6)


def measure(n_rows, calls):
    lib = _native.lib()
    sh = HipIndexShard(DIM, n_rows, 0)
    for blk in bench.synth_rows(0, n_rows):
        sh.append_rows(blk)
    assert sh._shadow is not None, "a shard of this size seals a shadow"
    nbytes = ctypes.c_size_t()
    _native.check(lib.emdr2_mips_block_norm_bytes(n_rows, ctypes.byref(nbytes)), "block_norm_bytes")
    norms = torch.empty(nbytes.value // 4, dtype=torch.float32, device=sh.device)
    _native.check(lib.emdr2_mips_block_norms(sh.tiled.data_ptr(), n_rows, DIM, 0, norms.numel(), norms.data_ptr(), _native.stream_ptr()), "block_norms")
    sh._block_norms = norms                                          # (what the first in-place update would have built)
    report = torch.empty(_native.AUDIT_WORDS, dtype=torch.int64, device=sh.device)
    image, table = sh._shadow
    b16, b8 = sh.tiled.numel(), image.numel()
    dst = torch.empty(b16 + b8, dtype=torch.uint8, device=sh.device)

    def audit(with_shadow):
        _native.check(lib.emdr2_mips_audit(sh.tiled.data_ptr(), n_rows, DIM, 0, sh.emax_sq.data_ptr(), norms.data_ptr(),
                                           image.data_ptr() if with_shadow else None, table.data_ptr() if with_shadow else None,
                                           report.data_ptr(), _native.stream_ptr()), "mips_audit")

    def copy(with_shadow):
        dst[:b16].copy_(sh.tiled)
        if with_shadow:
            dst[b16:].copy_(image)
    fns = (("audit16", lambda: audit(False)), ("copy16", lambda: copy(False)), ("audit24", lambda: audit(True)), ("copy24", lambda: copy(True)))
    t = {name: [] for name, _ in fns}
    for i in range(WARMUP + calls):
        for name, fn in fns:
            ms = timed_ms(fn)
            if i >= WARMUP:
                t[name].append(ms)
    words = [w & _native.AUDIT_NONE for w in report.tolist()]
    assert words[0] == n_rows and not any(words[1:12]), words       # what was timed was a clean audit of the whole shard
    wall = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = sh.audit()
        wall.append((time.perf_counter() - t0) * 1000.0)
    assert result["sound"] and result["canonical"] and result["shadow_in_use"]
    return ["%d rows x %d: fp16 image %.2f GB, int8 image %.2f GB" % (n_rows, DIM, b16 / 1e9, b8 / 1e9),
            rate_line("emdr2_mips_audit, fp16 words only (read)", t["audit16"], b16),
            rate_line("device-to-device copy of the fp16 image (read + written)", t["copy16"], 2 * b16),
            rate_line("emdr2_mips_audit with the shadow (read)", t["audit24"], b16 + b8),
            rate_line("device-to-device copy of both images (read + written)", t["copy24"], 2 * (b16 + b8)),
            "  HipIndexShard.audit() with the shadow, enqueue to read-back, wall clock: median %.3f ms of %d" % (statistics.median(wall), len(wall)),
            "  the audit with the shadow reads %.1f GB/s where the copy reads %.1f GB/s (and writes as much)"
            % ((b16 + b8) / statistics.median(t["audit24"]) / 1e6, (b16 + b8) / statistics.median(t["copy24"]) / 1e6)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[SHARD_ROWS, FULL_ROWS])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mips_audit.txt"))
    args = ap.parse_args()
    lines = ["tools/mips_audit_bench.py: %s, %d CUs, device events, %d warm-ups + %d timed calls per variant, alternating"
             % (torch.cuda.get_device_name(0), _native.lib().emdr2_device_cu_count(), WARMUP, args.calls)]
    for n in args.rows:
        lines += measure(n, args.calls)
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
