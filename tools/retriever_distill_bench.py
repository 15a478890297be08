"""Time what --retriever-distill-attention and --attention-mass-value-norms add to and remove from the training step
(profiles/retriever_distill.txt).

  python tools/retriever_distill_bench.py [--out FILE] [--no-step] [--rows N] [--steps N]

Part 1, the launches: BASELINE configs[2]'s decoder cross-attention of one question group -- 16 questions, 32 decoder positions, 12 heads
of 64 channels over the packed keys of K = 50 passages (about 400 real tokens each) -- and the K = 100 shape.  Device events around blocks
of back-to-back launches of (a) the split-key forward the mass kernel follows, (b) the unweighted `kernels.attention_key_mass`, (c) the
weighted one (`kw` = the value norms) and (d) `kernels.head_row_norms` over the V half of the packed KV projection; the four alternate,
medians over the blocks.

Part 2, the step: the end-to-end training step of bench_e2e.py (configs[2]: B = 64, K = 50, 12 layers) on ONE model in three modes,
alternating step by step after a warm-up: both switches off, `retriever_distill_attention`, and `retriever_distill_attention` with
`attention_mass_value_norms`; wall-clock per step with a device synchronisation on either side, median and spread per mode.  With the
switches off the step launches exactly what it launched before they existed, so the "off" column is the baseline; the spread of the
"off" steps is the yardstick for the differences.  No ratio is fixed in advance.

The new kernels' register counts (tools/kernel_resources.py) are appended."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from reader_mass_bench import BLOCK, REPS, timed  # noqa: E402

MODES = (("off", False, False), ("distill", True, False), ("distill + value norms", True, True))


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
        kw = torch.empty((heads, seqs.rows), device="cuda")

        def forward():
            with torch.no_grad():
                K.attention_core(q, kv, dec, gk, False)

        def plain():
            K.attention_key_mass(q, kv[:, 0], dec, gk, m, l, seg, w, mass)

        def norms():
            K.head_row_norms(kv[:, 1], out=kw)

        def weighted():
            K.attention_key_mass(q, kv[:, 0], dec, gk, m, l, seg, w, mass, kw=kw)
        fns = (("forward", forward), ("mass", plain), ("norms", norms), ("weighted mass", weighted))
        for _, fn in fns:
            timed(fn, BLOCK)
        res = {name: [] for name, _ in fns}
        for _ in range(REPS):
            for name, fn in fns:
                res[name].append(timed(fn, BLOCK))
        v_bytes = seqs.rows * heads * 64 * 2
        row = "K = %3d: %d questions x %d positions x %d heads over %d packed keys (%d rows), forward ksplit %d:" % (
            Kk, B, L, heads, seqs.total, seqs.rows, ksplit)
        for name, _ in fns:
            r = res[name]
            row += "  %s %.1f us [%.1f .. %.1f]" % (name, statistics.median(r), min(r), max(r))
        med = {name: statistics.median(res[name]) for name, _ in fns}
        row += "  weighted/mass %.2f  weighted/forward %.2f  norms %.0f GB/s of V" % (
            med["weighted mass"] / med["mass"], med["weighted mass"] / med["forward"], v_bytes / med["norms"] / 1e3)
        lines.append(row)
        print(row, flush=True)


def step_part(lines, rows, steps):
    import bench_e2e
    ap = argparse.ArgumentParser()
    bench_e2e.add_args(ap)
    args = ap.parse_args([])
    args.rows = rows
    ctx = bench_e2e.setup(args, 0, 1)
    model = ctx.model

    def switch(distill, norms):
        model.retriever_distill_attention, model.attention_mass_value_norms = distill, norms
    for i in range(3):                                                     # warm-up: allocator, sticky packed capacities, every mode once
        switch(*MODES[i][1:])
        ctx.step()
    times = {name: [] for name, _, _ in MODES}
    for i in range(len(MODES) * steps):
        name, distill, norms = MODES[i % len(MODES)]
        switch(distill, norms)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.step()
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) * 1000.0)
    switch(False, False)
    off = statistics.median(times["off"])
    lines.append("training step, B = %d, K = %d, %d layers, %d question groups, %d alternating steps per mode:" % (ctx.B, ctx.K, ctx.layers, ctx.guard.micro, steps))
    for name, _, _ in MODES:
        t = times[name]
        lines.append("  %-22s %.1f ms [%.1f .. %.1f], spread %.1f ms, against off %+.1f ms (%+.2f %%)"
                     % (name, statistics.median(t), min(t), max(t), max(t) - min(t), statistics.median(t) - off, 100.0 * (statistics.median(t) / off - 1.0)))
    for row in lines[-len(MODES) - 1:]:
        print(row, flush=True)


def register_part(lines):
    import kernel_resources as kr
    for e in sorted(kr.kernels(), key=lambda e: e["name"]):
        if "attention_key_mass_kernel" in e["name"] or "head_row_norms_kernel" in e["name"]:
            lines.append("kernel resources (tools/kernel_resources.py): %s %d VGPRs + %d AGPRs, %d SGPRs, spills %d / %d, private segment %d, LDS %d B"
                         % (e["name"], e["vgpr_count"], e["agpr_count"], e["sgpr_count"], e["vgpr_spill_count"], e["sgpr_spill_count"],
                            e["private_segment_fixed_size"], e["group_segment_fixed_size"]))
            print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--rows", type=int, default=400_000, help="rows of the synthetic evidence index behind the step (its search is not what is measured)")
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("retriever_distill_bench needs a GPU: there is nothing to measure without one")
    lines = ["retriever distillation from the reader's attention mass, %s" % torch.cuda.get_device_name(0),
             "launches: us per launch, median of %d alternating blocks of %d back-to-back launches [min .. max]" % (REPS, BLOCK), ""]
    launch_part(lines)
    if not args.no_step:
        lines.append("")
        step_part(lines, args.rows, args.steps)
    lines.append("")
    register_part(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
