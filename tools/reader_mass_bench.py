"""Time the reader attention mass (csrc/attention_mass.hip) next to the launch it observes, and the training step with the flag on and off
(profiles/reader_attention_mass.txt).

  python tools/reader_mass_bench.py [--out FILE] [--no-step] [--rows N] [--steps N]

Part 1, the launch: BASELINE configs[2]'s decoder cross-attention of one question group -- 16 questions, 32 decoder positions, 12 heads of
64 channels over the packed keys of K = 50 passages (about 400 real tokens each) -- and the K = 100 shape.  Device events around blocks of
back-to-back launches of (a) the split-key forward (`kernels.attention_core` under no_grad: the forward kernel and its combine kernel)
and (b) `kernels.attention_key_mass` on the same operands with that forward's statistics; the two alternate, medians over the blocks.

Part 2, the step: the end-to-end training step of bench_e2e.py (configs[2]: B = 64, K = 50, 12 layers) with `reader_attention_mass`
switched on and off on the SAME model, alternating step by step after a warm-up, wall-clock per step with a device synchronisation on
either side.  With the flag off the step launches exactly what it launched before the flag existed (tests/test_reader_mass_model_gpu.py:
bit-identical logits, loss and reproducible gradients), so the "off" column is the step without the feature; the spread of the "off" steps
is the yardstick for the difference."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BLOCK, REPS = 10, 15


def timed(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / launches          # microseconds per launch


def launch_part(lines):
    from emdr2_amd.model import kernels as K
    B, L, heads, S = 16, 32, 12, 512
    g = torch.Generator(device="cuda").manual_seed(3)
    for Kk in (50, 100):
        lens = torch.randint(300, 501, (B * Kk,), generator=g, device="cuda")
        ids = (torch.arange(S, device="cuda")[None] < lens[:, None]).to(torch.int64) * 7
        seqs = K.PackedSeqs(ids)
        gk = seqs.grouped(Kk)
        q = torch.randn((B, L, heads, 64), generator=g, device="cuda").bfloat16()
        kv = torch.randn((seqs.rows, 2, heads, 64), generator=g, device="cuda").bfloat16()
        dec = torch.full((B, L), 7, dtype=torch.int64, device="cuda")
        dec[:, 6:] = 0                                                     # answers of a few tokens: most decoder positions are padding
        idx = torch.arange(B, device="cuda")[:, None] * Kk + torch.arange(Kk + 1, device="cuda")[None]
        seg = (seqs.cu[idx] - seqs.cu[idx][:, :1]).to(torch.int32).contiguous()
        w = (dec != 0).float()
        out = K.attention_core(q.clone().requires_grad_(True), kv, dec, gk, False)
        m, l = (t.detach() for t in out.grad_fn.saved_tensors[2:4])
        ksplit = out.grad_fn.launch.ksplit
        mass = torch.zeros((B, heads, Kk), device="cuda")

        def forward():
            with torch.no_grad():
                K.attention_core(q, kv, dec, gk, False)

        def mass_launch():
            K.attention_key_mass(q, kv[:, 0], dec, gk, m, l, seg, w, mass)
        for fn in (forward, mass_launch):
            timed(fn, BLOCK)
        res = {"forward": [], "mass": []}
        for _ in range(REPS):
            res["forward"].append(timed(forward, BLOCK))
            res["mass"].append(timed(mass_launch, BLOCK))
        key_bytes = seqs.total * heads * 64 * 2
        row = "K = %3d: %d questions x %d positions x %d heads over %d packed keys (%.0f MB of K), forward ksplit %d:" % (
            Kk, B, L, heads, seqs.total, key_bytes / 1e6, ksplit)
        for name in ("forward", "mass"):
            r = res[name]
            row += "  %s %.1f us [%.1f .. %.1f]" % (name, statistics.median(r), min(r), max(r))
        med = statistics.median(res["mass"])
        row += "  mass/forward %.2f  (%.0f GB/s of keys)" % (med / statistics.median(res["forward"]), key_bytes / med / 1e3)
        lines.append(row)
        print(row, flush=True)


def step_part(lines, rows, steps):
    import bench_e2e
    ap = argparse.ArgumentParser()
    bench_e2e.add_args(ap)
    args = ap.parse_args([])
    args.rows = rows
    ctx = bench_e2e.setup(args, 0, 1)
    for _ in range(3):                                                     # warm-up: allocator, sticky packed capacities
        ctx.step()
    times = {False: [], True: []}
    for i in range(2 * steps):
        flag = bool(i % 2)
        ctx.model.reader_attention_mass = flag
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.step()
        torch.cuda.synchronize()
        times[flag].append((time.perf_counter() - t0) * 1000.0)
    ctx.model.reader_attention_mass = False
    off, on = times[False], times[True]
    row = ("training step, B = %d, K = %d, %d layers, %d question groups, %d alternating steps each: off %.1f ms [%.1f .. %.1f], on %.1f ms "
           "[%.1f .. %.1f], on - off %+.1f ms (%+.2f %%), spread of the off steps %.1f ms"
           % (ctx.B, ctx.K, ctx.layers, ctx.guard.micro, steps, statistics.median(off), min(off), max(off), statistics.median(on), min(on), max(on),
              statistics.median(on) - statistics.median(off), 100.0 * (statistics.median(on) / statistics.median(off) - 1.0), max(off) - min(off)))
    lines.append(row)
    print(row, flush=True)
    mass = ctx.model.last_attention_mass
    lines.append("last_attention_mass of the last flagged step: shape %s, row sums %.6f .. %.6f" % (tuple(mass.shape), float(mass.sum(1).min()), float(mass.sum(1).max())))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--rows", type=int, default=400_000, help="rows of the synthetic evidence index behind the step (its search is not what is measured)")
    ap.add_argument("--steps", type=int, default=6)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("reader_mass_bench needs a GPU: there is nothing to measure without one")
    lines = ["reader attention mass, %s" % torch.cuda.get_device_name(0),
             "launches: us per launch, median of %d alternating blocks of %d back-to-back launches [min .. max]" % (REPS, BLOCK), ""]
    launch_part(lines)
    if not args.no_step:
        lines.append("")
        step_part(lines, args.rows, args.steps)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
