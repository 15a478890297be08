#!/usr/bin/env python
"""Price of --skip-nonfinite-steps (FlatAdam(skip_nonfinite=True); include/emdr2_ops.h, "Step guard"), measured on the GPU in ONE process:
`FlatAdam.step()` at the benchmark's parameter count (440,388,096 fp32 masters in 512 MiB buckets), the guard on and off alternately on two
optimizers that hold the same number of elements and finite gradients -- the path every healthy step takes: the census rides in the
norm pass, one verdict launch, one 8-byte load per Adam thread.  A skipped step (one NaN planted) is timed as well: it reads the
gradients once and stores nothing.

    python tools/step_guard_bench.py [--params 440388096] [--rounds 9] > profiles/step_guard.txt

Times are device-event times around `inner` back-to-back steps, median over alternating rounds, after a warm-up of both arms."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(n_params, guard, chunk=1 << 22):
    """A FlatAdam over `n_params` elements in tensors of `chunk`, every tensor with a gradient this step (random, norm above the clip)."""
    from emdr2_amd.training import FlatAdam
    mod = torch.nn.Module()
    left, i = n_params, 0
    while left > 0:
        n = min(chunk, left)
        mod.register_parameter("p%d" % i, torch.nn.Parameter(torch.randn(n, device="cuda") * 0.02))
        left -= n; i += 1
    opt = FlatAdam(mod, lr=2e-5, weight_decay=0.1, clip_grad=1.0, skip_nonfinite=guard)
    gen = torch.Generator(device="cuda").manual_seed(1)
    for b in opt.buckets:
        b["grad"].copy_(torch.randn(b["n"], generator=gen, device="cuda") * 1e-3)
    for p in opt.params:                      # as after a backward that reached every parameter once
        opt.count[p] = 1
    opt.expected = dict(opt.count)
    return opt


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=440388096)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    a = ap.parse_args()
    arms = {"off": build(a.params, False), "on": build(a.params, True)}
    print("# FlatAdam.step(), %d parameters, %d buckets, %s" % (a.params, len(arms["on"].buckets), torch.cuda.get_device_name(0)))
    for opt in arms.values():
        opt.step(); opt.step()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, opt in arms.items():
            t[k].append(timed(opt.step, a.inner))
    med = {k: statistics.median(v) for k, v in t.items()}
    for k in arms:
        print("guard %-3s  %8.3f ms per step (min %.3f max %.3f)  %d launches" % (k, med[k], min(t[k]), max(t[k]), arms[k].optimizer_launches))
    print("on / off = %.4f  (+%.3f ms per step)" % (med["on"] / med["off"], med["on"] - med["off"]))
    rep = arms["on"].guard_report()
    assert rep["skipped_total"] == 0, rep
    # a skipped step: one NaN among the gradients
    on = arms["on"]
    on.buckets[-1]["grad"][12345] = float("nan")
    on.step()
    skipped = [timed(on.step, a.inner) for _ in range(a.rounds)]
    rep = on.guard_report()
    assert rep["skipped_total"] == 1 + a.rounds * a.inner and rep["nan"] == 1, rep
    print("skipped    %8.3f ms per step (min %.3f max %.3f)  first offender %s[%d]" % (statistics.median(skipped), min(skipped), max(skipped),
                                                                                       rep["parameter"], rep["element"]))


if __name__ == "__main__":
    main()
