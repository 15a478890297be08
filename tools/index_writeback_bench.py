"""Time of the scattered in-place row update behind --index-writeback next to the contiguous update of the same number of rows.

What a step boundary hands the index at B = 64, K = 50: 3,200 rows on one rank, or the gathered 25,600 rows of eight ranks of which an
eighth fall into this rank's shard (the others are skipped on the device).  Both lists spread uniformly over an N / 8 shard and over the
full index, dim 768, int8 shadow sealed.  `HipIndexShard.update_rows_at` (duplicate resolution, the C entry, the flag read-back), the C
entry `emdr2_mips_update_rows_scattered` alone, and `emdr2_mips_update_rows` of 3,200 contiguous rows -- the same bytes written, 13 - 14
blocks re-sealed instead of up to 3,200 -- alternating call by call in one process.  Device events around each call, 3 warm-ups, then
`--calls` timed calls; median, min and max in microseconds.  The registers of the new kernels come from tools/kernel_resources.py.
usage: python tools/index_writeback_bench.py [--rows 2626916 21015324] [--calls 20] [--out profiles/index_writeback.txt]"""
import argparse
import ctypes
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

import bench  # noqa: E402
import kernel_resources as kr  # noqa: E402
from emdr2_amd import _native  # noqa: E402
from emdr2_amd.data.emdr2_index import HipIndexShard  # noqa: E402

DIM, OWN, GATHERED, WARMUP = 768, 3200, 25600, 3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0


def line(name, us):
    return "  %-66s median %9.1f us   min %9.1f   max %9.1f   (%d calls)" % (name, statistics.median(us), min(us), max(us), len(us))


def measure(n_rows, calls):
    lib = _native.lib()
    sh = HipIndexShard(DIM, n_rows, 0)
    for blk in bench.synth_rows(0, n_rows):
        sh.append_rows(blk)
    assert sh._shadow is not None
    g = torch.Generator(device="cuda").manual_seed(99)
    rows = torch.randn((GATHERED, DIM), generator=g, device="cuda").half()
    own = torch.randperm(n_rows, generator=g, device="cuda")[:OWN]                     # distinct, uniform over the shard
    gathered = n_rows + torch.randint(0, 7 * n_rows, (GATHERED,), generator=g, device="cuda")    # rows of the other seven shards ...
    gathered[torch.randperm(GATHERED, generator=g, device="cuda")[:OWN]] = own          # ... and an eighth of this one, anywhere in the list
    stream = _native.stream_ptr()
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    sh.update_rows(0, rows[:1])                                                         # (builds the block-norm table)
    ws_bytes = ctypes.c_size_t()
    _native.check(lib.emdr2_mips_scatter_workspace_bytes(n_rows, GATHERED, ctypes.byref(ws_bytes)), "scatter_workspace_bytes")
    ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device="cuda")
    lo = n_rows // 2 + 3

    def entry(ids):
        return lambda: _native.check(lib.emdr2_mips_update_rows_scattered(
            rows.data_ptr(), ids.data_ptr(), ids.numel(), DIM, n_rows, sh.tiled.data_ptr(), sh._block_norms.data_ptr(), sh.emax_sq.data_ptr(),
            sh._shadow[0].data_ptr(), sh._shadow[1].data_ptr(), bad.data_ptr(), ws.data_ptr(), ws.numel(), stream), "update_rows_scattered")
    contiguous = lambda: _native.check(lib.emdr2_mips_update_rows(rows.data_ptr(), OWN, DIM, lo, n_rows, sh.tiled.data_ptr(), sh._block_norms.data_ptr(),
                                                                  sh.emax_sq.data_ptr(), sh._shadow[0].data_ptr(), sh._shadow[1].data_ptr(), bad.data_ptr(),
                                                                  stream), "update_rows")
    cases = (("update_rows_at, %d rows (incl. duplicate resolution, flag read-back)" % OWN, lambda: sh.update_rows_at(own, rows[:OWN])),
             ("emdr2_mips_update_rows_scattered alone, %d rows" % OWN, entry(own)),
             ("update_rows_at, %d gathered rows, %d in the shard" % (GATHERED, OWN), lambda: sh.update_rows_at(gathered, rows)),
             ("emdr2_mips_update_rows_scattered alone, %d gathered rows" % GATHERED, entry(gathered)),
             ("emdr2_mips_update_rows alone, %d contiguous rows" % OWN, contiguous))
    t = [[] for _ in cases]
    for i in range(WARMUP + calls):                                      # alternating, so that clocks and caches treat all alike
        for j, (_, fn) in enumerate(cases):
            us = timed(fn)
            if i >= WARMUP:
                t[j].append(us)
    touched = int(torch.unique(own // 256).numel())
    out = ["%d rows x %d, int8 shadow sealed; %d scattered rows touch %d blocks of 256, %d contiguous rows at row %d touch %d; workspace %d bytes"
           % (n_rows, DIM, OWN, touched, OWN, lo, (lo + OWN - 1) // 256 - lo // 256 + 1, ws_bytes.value)]
    out += [line(name, us) for (name, _), us in zip(cases, t)]
    out.append("  ratio scattered entry / contiguous entry at %d rows, medians: %.2f" % (OWN, statistics.median(t[1]) / statistics.median(t[4])))
    assert int(bad.item()) == 0 and sh._shadow is not None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[2626916, 21015324])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_writeback.txt"))
    args = ap.parse_args()
    with open(_native.LIB_PATH, "rb") as fh:
        sha = hashlib.sha256(fh.read()).hexdigest()
    text = ["scattered in-place row update (--index-writeback) vs the contiguous update (tools/index_writeback_bench.py); device: %s; "
            "libemdr2_hip.so sha256 %s" % (torch.cuda.get_device_name(0), sha)]
    for n in args.rows:
        text += [""] + measure(n, args.calls)
        torch.cuda.empty_cache()
    text += ["", "registers of the kernels of a scattered update (tools/kernel_resources.py): vgpr, agpr, sgpr, vgpr spills, scratch bytes"]
    for e in kr.kernels():
        if any(s in e["name"] for s in ("pack_rows_at_kernel", "block_norms_kernel", "seal_shadow_kernel", "table_max_kernel")):
            text.append("  %4d %4d %4d %4d %6d  %s" % (e["vgpr_count"], e["agpr_count"], e["sgpr_count"], e["vgpr_spill_count"],
                                                    e["private_segment_fixed_size"], e["name"]))
    text = "\n".join(text) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
