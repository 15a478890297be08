"""Cost of generation stamps (--index-generations / --index-newest-wins): the stamped in-place updates next to the unstamped ones at the two
step-boundary shapes of e2e_k100, and one whole-shard statistics pass.

On an N / 8 shard, dim 768, int8 shadow sealed: `emdr2_mips_update_rows` against `emdr2_mips_update_rows_stamped` of 5,376 contiguous rows
(what the rolling refresher applies at a boundary), and `emdr2_mips_update_rows_scattered` against `_scattered_stamped` of 64 x 100 distinct
rows spread over the shard (the write-back), each stamped form with newest-wins off, on with every row admitted, and on with every row newer
(nothing is written); then `emdr2_mips_generation_stats` over the whole shard and over a 512 x 100 hit list.  C entries only, alternating
call by call in one process.  Device events around each call, 3 warm-ups, then `--calls` timed calls; median, min and max in microseconds.
The registers of the kernels come from tools/kernel_resources.py.
usage: python tools/index_generations_bench.py [--rows 2626916] [--calls 20] [--out profiles/index_generations.txt]"""
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
from index_writeback_bench import line, timed  # noqa: E402

DIM, RANGE, LIST, HITS, WARMUP = 768, 5376, 64 * 100, 512 * 100, 3


def measure(n_rows, calls):
    lib = _native.lib()
    sh = HipIndexShard(DIM, n_rows, 0, generations=True)
    for blk in bench.synth_rows(0, n_rows):
        sh.append_rows(blk)
    assert sh._shadow is not None
    g = torch.Generator(device="cuda").manual_seed(99)
    rows = torch.randn((LIST, DIM), generator=g, device="cuda").half()
    ids = torch.randperm(n_rows, generator=g, device="cuda")[:LIST]                    # distinct, uniform over the shard
    hits = torch.randint(0, 8 * n_rows, (HITS,), generator=g, device="cuda")            # an eighth falls into this shard
    stream = _native.stream_ptr()
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    sh.update_rows(0, rows[:1], generation=0)                                           # (builds the block-norm table)
    ws_bytes = ctypes.c_size_t()
    _native.check(lib.emdr2_mips_scatter_workspace_bytes(n_rows, LIST, ctypes.byref(ws_bytes)), "scatter_workspace_bytes")
    ws = torch.empty(ws_bytes.value, dtype=torch.uint8, device="cuda")
    report = torch.empty(_native.GEN_WORDS, dtype=torch.int64, device="cuda")
    lo = n_rows // 2 + 3
    sh.generation.fill_(5)
    head = (sh.tiled.data_ptr(), sh._block_norms.data_ptr(), sh.emax_sq.data_ptr(), sh._shadow[0].data_ptr(), sh._shadow[1].data_ptr(), bad.data_ptr())
    stamp = lambda gen, newest: (sh.generation.data_ptr(), gen, newest, sh._kept_newer.data_ptr())

    def range_plain():
        _native.check(lib.emdr2_mips_update_rows(rows.data_ptr(), RANGE, DIM, lo, n_rows, *head, stream), "update_rows")

    def range_stamped(gen, newest):
        return lambda: _native.check(lib.emdr2_mips_update_rows_stamped(rows.data_ptr(), RANGE, DIM, lo, n_rows, *head, *stamp(gen, newest), stream),
                                     "update_rows_stamped")

    def list_plain():
        _native.check(lib.emdr2_mips_update_rows_scattered(rows.data_ptr(), ids.data_ptr(), LIST, DIM, n_rows, *head, ws.data_ptr(), ws.numel(), stream),
                      "update_rows_scattered")

    def list_stamped(gen, newest):
        return lambda: _native.check(lib.emdr2_mips_update_rows_scattered_stamped(
            rows.data_ptr(), ids.data_ptr(), LIST, DIM, n_rows, *head, ws.data_ptr(), ws.numel(), *stamp(gen, newest), stream), "update_rows_scattered_stamped")

    def stats(rows_ptr, n_sel):
        return lambda: _native.check(lib.emdr2_mips_generation_stats(sh.generation.data_ptr(), n_rows, 0, rows_ptr, n_sel, 9, report.data_ptr(), stream),
                                     "generation_stats")
    # (every stamped call writes generation 5 over stamps of 5, or meets them with 4: the stamps are the same before every call)
    cases = (("emdr2_mips_update_rows, %d contiguous rows" % RANGE, range_plain),
             ("emdr2_mips_update_rows_stamped, newest_wins off", range_stamped(5, 0)),
             ("emdr2_mips_update_rows_stamped, newest_wins on, every row written", range_stamped(5, 1)),
             ("emdr2_mips_update_rows_stamped, newest_wins on, every row newer", range_stamped(4, 1)),
             ("emdr2_mips_update_rows_scattered, %d scattered rows" % LIST, list_plain),
             ("emdr2_mips_update_rows_scattered_stamped, newest_wins off", list_stamped(5, 0)),
             ("emdr2_mips_update_rows_scattered_stamped, newest_wins on, every row written", list_stamped(5, 1)),
             ("emdr2_mips_update_rows_scattered_stamped, newest_wins on, every row newer", list_stamped(4, 1)),
             ("emdr2_mips_generation_stats, the whole shard", stats(None, 0)),
             ("emdr2_mips_generation_stats, %d hits of which an eighth in the shard" % HITS, stats(hits.data_ptr(), HITS)))
    t = [[] for _ in cases]
    for i in range(WARMUP + calls):                                      # alternating, so that clocks and caches treat all alike
        for j, (_, fn) in enumerate(cases):
            us = timed(fn)
            if i >= WARMUP:
                t[j].append(us)
    med = [statistics.median(us) for us in t]
    out = ["%d rows x %d, int8 shadow sealed; %d contiguous rows at row %d touch %d blocks of 256, %d scattered rows touch %d"
           % (n_rows, DIM, RANGE, lo, (lo + RANGE - 1) // 256 - lo // 256 + 1, LIST, int(torch.unique(ids // 256).numel()))]
    out += [line(name, us) for (name, _), us in zip(cases, t)]
    out.append("  ratio stamped (newest_wins on, every row written) / unstamped, medians: contiguous %.3f, scattered %.3f" % (med[2] / med[0], med[6] / med[4]))
    kept = sh.kept_newer()
    assert kept == (WARMUP + calls) * (RANGE + LIST), kept               # exactly the "every row newer" calls were left alone
    assert int(bad.item()) == 0 and sh._shadow is not None and int((sh.generation[:n_rows] != 5).sum()) == 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[2626916])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_generations.txt"))
    args = ap.parse_args()
    with open(_native.LIB_PATH, "rb") as fh:
        sha = hashlib.sha256(fh.read()).hexdigest()
    text = ["generation-stamped in-place row updates vs the unstamped ones, and the statistics pass (tools/index_generations_bench.py); "
            "device: %s; libemdr2_hip.so sha256 %s" % (torch.cuda.get_device_name(0), sha)]
    for n in args.rows:
        text += [""] + measure(n, args.calls)
        torch.cuda.empty_cache()
    text += ["", "registers of the kernels (tools/kernel_resources.py): vgpr, agpr, sgpr, vgpr spills, scratch bytes"]
    for e in kr.kernels():
        if any(s in e["name"] for s in ("pack_rows_kernel", "pack_rows_at_kernel", "generation_stats")):
            text.append("  %4d %4d %4d %4d %6d  %s" % (e["vgpr_count"], e["agpr_count"], e["sgpr_count"], e["vgpr_spill_count"],
                                                    e["private_segment_fixed_size"], e["name"]))
    text = "\n".join(text) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
