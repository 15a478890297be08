"""--context-embeddings-from-index, measured: the EMDR2 training step with the context encoder frozen, WITHOUT and WITH the mode, in one
process on one device.

arm A   no_context_embedder_training=True, disable_retriever_dropout=True: the frozen context tower still runs its forward over the
        B x K retrieved passages (the step as it was before the flag existed, and the flag off)
arm B   the same with context_embeddings_from_index=True: one gather launch + the fp16-context prior instead of that forward

Both arms run on ONE model / optimizer / index (bench_e2e.setup); the arm is a switch read at the start of each forward.  The arms alternate
step by step after `--warmup` steps of each; every timed step ends in a device synchronise and is timed by the host clock.  Per arm: median,
min, max and the inter-quartile range of the step, peak HBM (the allocator's peak, reset before every step), and -- from device events around
the calls, summed over the step's question groups -- the context tower's forward (arm A), the gather and the prior's forward launch (arm B).
A step inside which a packed stack grew its sticky row capacity, or the caching allocator had to retry, is listed but not counted: the
rule of bench_e2e.run, which times its steps again after such an event.

shapes  configs[2]: B = 64, top-k 50, the full 21,015,324-row index, dropout 0.1, the benchmark's question grouping
        configs[4] per rank: top-k 100 over a ceil(N / 8)-row shard, 8 question groups
usage: python tools/context_from_index_ab.py [--steps 10] [--warmup 2] [--rows N] [--batch B] [--layers L] [--shapes k50 k100]
                                             [--out profiles/context_from_index.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench_e2e  # noqa: E402
from emdr2_amd.model import kernels as K  # noqa: E402


class EventSpans(object):
    """device time of the wrapped calls, read after the step's synchronise"""

    def __init__(self):
        self.pairs = []

    def wrap(self, fn, when=lambda *a, **kw: True):
        def timed(*a, **kw):
            if not when(*a, **kw):
                return fn(*a, **kw)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **kw)
            e1.record()
            self.pairs.append((e0, e1))
            return out
        return timed

    def take_ms(self):
        ms = sum(a.elapsed_time(b) for a, b in self.pairs)
        self.pairs = []
        return ms


def quartiles(v):
    q = statistics.quantiles(v, n=4) if len(v) >= 4 else [min(v), statistics.median(v), max(v)]
    return q[0], q[2]


def ab(a, topk, rows, steps, warmup):
    index = bench_e2e.build_index(rows, 0, 1)
    ctx = bench_e2e.setup(a, 0, 1, index=index, topk=topk)
    model, retr = ctx.model, ctx.retriever
    model.no_context_embedder_training = True                            # both arms: the frozen context encoder of the reference's switch
    model.disable_retriever_dropout = True
    tower, gather, prior = EventSpans(), EventSpans(), EventSpans()
    model.retriever_embedder = tower.wrap(model.retriever_embedder, when=lambda tokens, mask, types_, kind, *r, **kw: kind == "context")
    retr.kept_embeddings = gather.wrap(retr.kept_embeddings)
    inner_prior = K.retriever_prior_h16
    K.retriever_prior_h16 = prior.wrap(inner_prior)
    t = {False: [], True: []}
    parts = {False: [], True: []}
    grew = {False: [], True: []}
    peak = {False: 0, True: 0}
    retries = lambda: int(torch.cuda.memory_stats().get("num_alloc_retries", 0))
    try:
        for i in range(warmup + steps):
            for mode in (False, True):
                model.context_embeddings_from_index = mode
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                before = (K.PACKING.growths, retries())
                t0 = time.perf_counter()
                ctx.step()
                torch.cuda.synchronize()
                ms = (time.perf_counter() - t0) * 1e3
                spans = (tower.take_ms(), gather.take_ms(), prior.take_ms())
                print("top-k %d step %d arm %s: %.1f ms" % (topk, i, "B" if mode else "A", ms), file=sys.stderr, flush=True)
                if i >= warmup and (K.PACKING.growths, retries()) != before:
                    # bench_e2e.run's rule: a packed stack that met a new maximum of real tokens grew its sticky row capacity inside this
                    # step (every activation size of the stack changes, none of the cached blocks fit: fresh allocations, about a second),
                    # or the allocator had to give blocks back and ask again.  That is warm-up, not the step: listed, not counted.
                    grew[mode].append(ms)
                elif i >= warmup:
                    t[mode].append(ms)
                    parts[mode].append(spans)
                    peak[mode] = max(peak[mode], torch.cuda.max_memory_allocated())
    finally:
        K.retriever_prior_h16 = inner_prior
    lines = ["B = %d, top-k %d, %d-row index, %d layers, dropout %.2f, %d question groups; %d warm-up + %d timed steps per arm, alternating"
             % (a.batch, topk, rows, a.layers, a.dropout, ctx.guard.micro, warmup, steps)]
    med = {}
    for mode, name in ((False, "A  context tower forward (flag off)"), (True, "B  rows from the index (flag on)  ")):
        v = t[mode]
        q1, q3 = quartiles(v)
        med[mode] = statistics.median(v)
        lines.append("  arm %s  median %8.1f ms  min %8.1f  max %8.1f  IQR %6.1f  peak HBM %6.1f GB   steps: %s%s"
                     % (name, med[mode], min(v), max(v), q3 - q1, peak[mode] / 1e9, " ".join("%.0f" % x for x in v),
                        ("   not counted (packed capacity grew / allocator retried inside the step): " + " ".join("%.0f" % x for x in grew[mode]))
                        if grew[mode] else ""))
    pa, pb = parts[False], parts[True]
    lines.append("  arm A  context tower forward, device events, per step: median %.1f ms" % statistics.median(p[0] for p in pa))
    lines.append("  arm B  gather (kept_embeddings) %.3f ms, prior forward (retriever_prior_h16, %d launches) %.3f ms per step; context tower %.1f ms"
                 % (statistics.median(p[1] for p in pb), ctx.guard.micro, statistics.median(p[2] for p in pb), statistics.median(p[0] for p in pb)))
    qa1, qa3 = quartiles(t[False])
    spread = max(t[False]) - min(t[False])
    saved = med[False] - med[True]
    lines.append("  B is faster than A by %.1f ms per step (%.1f %% of A); A's step-to-step spread: IQR %.1f ms, max - min %.1f ms -> %s"
                 % (saved, 100.0 * saved / med[False], qa3 - qa1, spread,
                    "faster by more than A's spread" if saved > spread else ("faster by more than A's IQR only" if saved > qa3 - qa1 else "NOT faster beyond A's spread")))
    del ctx, model, retr, index
    bench_e2e.release()
    return lines


def main():
    ap = argparse.ArgumentParser()
    bench_e2e.add_args(ap)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=21_015_324)
    ap.add_argument("--shapes", nargs="+", default=["k50", "k100"], choices=["k50", "k100"])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    full_rows = a.rows
    lines = ["--context-embeddings-from-index: the training step with the frozen context encoder, flag off (A) vs on (B); %s"
             % torch.cuda.get_device_name(0)]
    if "k50" in a.shapes:
        lines += ab(a, 50, full_rows, a.steps, a.warmup)
    if "k100" in a.shapes:
        a.micro_batches = 8
        a.rows = (full_rows + 7) // 8
        lines += ab(a, 100, a.rows, a.steps, a.warmup)
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
