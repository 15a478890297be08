"""Time of an in-place row update of the MIPS index next to the swap refresh's write of the same rows.

One `HipIndexShard.update_rows` of 5,376 rows (a 42-batch pump of the side-stream refresher) at dim 768 on a shard with a sealed int8
shadow, the C entry `emdr2_mips_update_rows` alone (no flag read-back), and `emdr2_mips_pack_rows` of the same rows into a spare image --
the body of `refresh_rows`, the only yardstick there is for the same bytes -- alternating call by call in one process; plus the one-off
build of the block-norm table.  Device events around each call, 3 warm-ups, then `--calls` timed calls; median, min and max in microseconds.
usage: python tools/mips_update_rows_bench.py [--rows 2626916 21015324] [--calls 20] [--out profiles/mips_update_rows.txt]"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402
from emdr2_amd import _native  # noqa: E402
from emdr2_amd.data.emdr2_index import HipIndexShard  # noqa: E402

DIM, CHUNK, WARMUP = 768, 5376, 3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0


def line(name, us):
    return "  %-58s median %9.1f us   min %9.1f   max %9.1f   (%d calls)" % (name, statistics.median(us), min(us), max(us), len(us))


def measure(n_rows, calls):
    lib = _native.lib()
    sh = HipIndexShard(DIM, n_rows, 0)
    for blk in bench.synth_rows(0, n_rows):
        sh.append_rows(blk)
    assert sh._shadow is not None
    spare, spare_emax = torch.zeros_like(sh.tiled), torch.zeros_like(sh.emax_sq)
    g = torch.Generator(device="cuda").manual_seed(99)
    rows = torch.randn((CHUNK, DIM), generator=g, device="cuda").half()
    lo = n_rows // 2 + 3                                                 # not block aligned: 22 blocks of 256 rows are touched
    stream = _native.stream_ptr()
    out = ["%d rows x %d, int8 shadow sealed; %d rows written at row %d (%d blocks of 256 touched)" %
           (n_rows, DIM, CHUNK, lo, (lo + CHUNK - 1) // 256 - lo // 256 + 1)]
    table_bytes = ctypes.c_size_t()
    _native.check(lib.emdr2_mips_block_norm_bytes(n_rows, ctypes.byref(table_bytes)), "block_norm_bytes")
    table = torch.empty(table_bytes.value // 4, dtype=torch.float32, device="cuda")
    build = lambda: _native.check(lib.emdr2_mips_block_norms(sh.tiled.data_ptr(), n_rows, DIM, 0, table.numel(), table.data_ptr(), stream), "block_norms")
    us = [timed(build) for _ in range(WARMUP + calls)][WARMUP:]
    out.append(line("block-norm table, one-off build (%d entries)" % table.numel(), us))
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    method = lambda: sh.update_rows(lo, rows)
    entry = lambda: _native.check(lib.emdr2_mips_update_rows(rows.data_ptr(), CHUNK, DIM, lo, n_rows, sh.tiled.data_ptr(), sh._block_norms.data_ptr(),
                                                             sh.emax_sq.data_ptr(), sh._shadow[0].data_ptr(), sh._shadow[1].data_ptr(), bad.data_ptr(),
                                                             stream), "update_rows")
    pack = lambda: _native.check(lib.emdr2_mips_pack_rows(rows.data_ptr(), CHUNK, DIM, lo, n_rows, spare.data_ptr(), spare_emax.data_ptr(), stream),
                                 "pack_rows")
    t = {"method": [], "entry": [], "pack": []}
    for i in range(WARMUP + calls):                                      # alternating, so that clocks and caches treat the three alike
        for name, fn in (("method", method), ("entry", entry), ("pack", pack)):
            us = timed(fn)
            if i >= WARMUP:
                t[name].append(us)
    out.append(line("HipIndexShard.update_rows (incl. the flag read-back)", t["method"]))
    out.append(line("emdr2_mips_update_rows alone (4 launches)", t["entry"]))
    out.append(line("emdr2_mips_pack_rows into a spare image (refresh_rows)", t["pack"]))
    out.append("  ratio update entry / pack_rows, medians: %.2f" % (statistics.median(t["entry"]) / statistics.median(t["pack"])))
    assert int(bad.item()) == 0 and sh._shadow is not None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[2626916, 21015324])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mips_update_rows.txt"))
    args = ap.parse_args()
    text = ["in-place row update vs the swap refresh's write of the same rows (tools/mips_update_rows_bench.py); device: %s"
            % torch.cuda.get_device_name(0)]
    for n in args.rows:
        text += [""] + measure(n, args.calls)
        torch.cuda.empty_cache()
    text = "\n".join(text) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
