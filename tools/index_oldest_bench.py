"""Cost of the oldest-first row selection (--index-refresh-oldest-first): `emdr2_mips_oldest_rows` at n_want = 5,376 (the rows the rolling
refresher embeds per step at e2e_k100) next to the whole-shard `emdr2_mips_generation_stats` pass and a device-to-device copy of the stamp
array, on the N / 8 shard's 2,626,916 stamps and the full index's 21,015,324.

The selection makes p = 5 passes over the stamps (three digit histograms, the per-slab counts, the ordered write; the write pass reads
only the slabs that hold a selected row), in six launches: on clustered stamps about five times the statistics pass is what to expect.
Stamp patterns: uniform (a fresh start: the selection is the first 5,376 rows); "refresher + write-back" (a pass half done: the first half
of the shard carries generation 400, the second half 0, and 2 % of all rows, anywhere, a write-back stamp in 400..450) with below = 400;
random 31-bit values (no digit of the select is trivial) with below = 2^31.  The three things alternate call by call in one process;
device events around each call, 3 warm-ups, then `--calls` timed calls; median, min and max in microseconds.

The per-step effect on the writer: on the N / 8 shard (dim 768, int8 shadow sealed) `emdr2_mips_update_rows_stamped` over a 5,376-row range
(the sequential refresher's boundary) against `emdr2_mips_update_rows_scattered_stamped` over 5,376 ascending rows -- the contiguous list a
uniform index gives, and the list the "refresher + write-back" pattern gives.  `--no-writer` leaves that part out (it builds the shard).
usage: python tools/index_oldest_bench.py [--rows 2626916 21015324] [--calls 20] [--no-writer] [--out profiles/index_oldest.txt]"""
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

DIM, WANT, WARMUP, PASSES = 768, 5376, 3, 5


def patterns(n_rows):
    """-> [(name, CUDA int32 stamps, below)]"""
    g = torch.Generator(device="cuda").manual_seed(7)
    uniform = torch.full((n_rows,), 400, dtype=torch.int32, device="cuda")
    mixed = torch.zeros(n_rows, dtype=torch.int32, device="cuda")
    mixed[:n_rows // 2] = 400
    recent = torch.randperm(n_rows, generator=g, device="cuda")[:n_rows // 50]
    mixed[recent] = torch.randint(400, 451, (recent.numel(),), generator=g, device="cuda", dtype=torch.int32)
    rand = torch.randint(0, 1 << 31, (n_rows,), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
    return [("uniform stamps (400), below 401", uniform, 401), ("refresher + write-back (0 / 400 / 400..450), below 400", mixed, 400),
            ("random 31-bit stamps, below 2^31", rand, 1 << 31)]


def alternate(cases, calls):
    t = [[] for _ in cases]
    for i in range(WARMUP + calls):                                      # alternating, so that clocks and caches treat all alike
        for j, (_, fn) in enumerate(cases):
            us = timed(fn)
            if i >= WARMUP:
                t[j].append(us)
    return t


def measure_select(n_rows, calls):
    lib = _native.lib()
    stream = _native.stream_ptr()
    nbytes = ctypes.c_size_t()
    _native.check(lib.emdr2_mips_oldest_rows_workspace_bytes(n_rows, ctypes.byref(nbytes)), "oldest_rows_workspace_bytes")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    rows = torch.empty(WANT, dtype=torch.int64, device="cuda")
    info = torch.empty(4, dtype=torch.int64, device="cuda")
    report = torch.empty(_native.GEN_WORDS, dtype=torch.int64, device="cuda")
    out = ["%d stamps (%.1f MB), n_want %d, workspace %d bytes" % (n_rows, n_rows * 4 / 1e6, WANT, nbytes.value)]
    lists = {}
    for name, stamps, below in patterns(n_rows):
        copy = torch.empty_like(stamps)

        def select():
            _native.check(lib.emdr2_mips_oldest_rows(stamps.data_ptr(), n_rows, 0, below, WANT, rows.data_ptr(), info.data_ptr(), ws.data_ptr(),
                                                     ws.numel(), stream), "oldest_rows")

        def stats():
            _native.check(lib.emdr2_mips_generation_stats(stamps.data_ptr(), n_rows, 0, None, 0, 500, report.data_ptr(), stream), "generation_stats")
        cases = (("emdr2_mips_oldest_rows", select), ("emdr2_mips_generation_stats, the whole shard", stats),
                 ("device-to-device copy of the stamps", lambda: copy.copy_(stamps)))
        t = alternate(cases, calls)
        med = [statistics.median(us) for us in t]
        words = info.tolist()
        out.append(" %s: selected %d of %d eligible, largest stamp selected %d" % (name, words[0], words[1], words[2]))
        out += [line(c[0], us) for c, us in zip(cases, t)]
        out.append("  ratio selection / statistics pass, medians: %.2f (p = %d passes over the stamps); selection / copy: %.2f"
                   % (med[0] / med[1], PASSES, med[0] / med[2]))
        lists[name] = rows.clone()
    return out, lists


def measure_writer(n_rows, calls, gappy):
    """the boundary's write: a 5,376-row range against 5,376 ascending rows through the scattered writer"""
    lib = _native.lib()
    stream = _native.stream_ptr()
    sh = HipIndexShard(DIM, n_rows, 0, generations=True)
    for blk in bench.synth_rows(0, n_rows):
        sh.append_rows(blk)
    assert sh._shadow is not None
    g = torch.Generator(device="cuda").manual_seed(99)
    new = torch.randn((WANT, DIM), generator=g, device="cuda").half()
    sh.update_rows(0, new[:1], generation=0)                             # (builds the block-norm table)
    sh.generation.fill_(5)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = ctypes.c_size_t()
    _native.check(lib.emdr2_mips_scatter_workspace_bytes(n_rows, WANT, ctypes.byref(nbytes)), "scatter_workspace_bytes")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    lo = n_rows // 2 + 3
    contiguous = torch.arange(lo, lo + WANT, dtype=torch.int64, device="cuda")
    head = (sh.tiled.data_ptr(), sh._block_norms.data_ptr(), sh.emax_sq.data_ptr(), sh._shadow[0].data_ptr(), sh._shadow[1].data_ptr(), bad.data_ptr())
    stamp = (sh.generation.data_ptr(), 5, 1, sh._kept_newer.data_ptr())

    def by_range():
        _native.check(lib.emdr2_mips_update_rows_stamped(new.data_ptr(), WANT, DIM, lo, n_rows, *head, *stamp, stream), "update_rows_stamped")

    def by_list(ids):
        return lambda: _native.check(lib.emdr2_mips_update_rows_scattered_stamped(new.data_ptr(), ids.data_ptr(), WANT, DIM, n_rows, *head, ws.data_ptr(),
                                                                                  ws.numel(), *stamp, stream), "update_rows_scattered_stamped")
    blocks = lambda ids: int(torch.unique(ids // 256).numel())
    cases = (("emdr2_mips_update_rows_stamped, a %d-row range" % WANT, by_range),
             ("emdr2_mips_update_rows_scattered_stamped, the same rows as a list (%d blocks)" % blocks(contiguous), by_list(contiguous)),
             ("..., the refresher + write-back selection (%d blocks)" % blocks(gappy), by_list(gappy)))
    t = alternate(cases, calls)
    med = [statistics.median(us) for us in t]
    out = ["%d rows x %d, int8 shadow sealed, newest-wins on, every row written" % (n_rows, DIM)]
    out += [line(c[0], us) for c, us in zip(cases, t)]
    out.append("  list / range, medians: %.3f (contiguous), %.3f (selection): +%.1f us / +%.1f us per step boundary"
               % (med[1] / med[0], med[2] / med[0], med[1] - med[0], med[2] - med[0]))
    assert int(bad.item()) == 0 and sh._shadow is not None and sh.kept_newer() == 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[2626916, 21015324])
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-writer", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_oldest.txt"))
    args = ap.parse_args()
    with open(_native.LIB_PATH, "rb") as fh:
        sha = hashlib.sha256(fh.read()).hexdigest()
    text = ["oldest-first row selection next to the statistics pass and a copy of the stamps (tools/index_oldest_bench.py); device: %s; "
            "libemdr2_hip.so sha256 %s" % (torch.cuda.get_device_name(0), sha)]
    gappy = None
    for n in args.rows:
        out, lists = measure_select(n, args.calls)
        text += [""] + out
        if gappy is None:
            gappy = [v for k, v in lists.items() if k.startswith("refresher")][0]
        torch.cuda.empty_cache()
    if not args.no_writer:
        text += [""] + measure_writer(args.rows[0], args.calls, gappy)
    text += ["", "registers of the kernels (tools/kernel_resources.py): vgpr, agpr, sgpr, vgpr spills, scratch bytes, LDS bytes"]
    for e in kr.kernels():
        if "oldest_" in e["name"]:
            text.append("  %4d %4d %4d %4d %6d %6d  %s" % (e["vgpr_count"], e["agpr_count"], e["sgpr_count"], e["vgpr_spill_count"],
                                                         e["private_segment_fixed_size"], e["group_segment_fixed_size"], e["name"]))
    text = "\n".join(text) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
