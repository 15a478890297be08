#!/usr/bin/env python
"""Price of one pass of parameter statistics (--log-param-stats-interval; FlatAdam.param_stats(), include/emdr2_ops.h, "Parameter
statistics"), measured on the GPU in ONE process at the benchmark's parameter count (440,388,096 elements in 512 MiB buckets): the two
launches of emdr2_param_stats per bucket -- 16 bytes per element read once, plus the records -- and, alternating with it in the same run,
emdr2_state_audit over the same buckets (14 bytes per element), the project's streaming pass next door and the yardstick here.  Then
FlatAdam.param_stats() as the task calls it, by the host clock: the launches, its one host read and the dict.

    python tools/param_stats_bench.py [--params 440388096] [--rounds 9] [--step-ms 1534] > profiles/param_stats.txt

Kernel times are device-event times around `inner` back-to-back passes over all buckets, median over alternating rounds, after a warm-up
of both arms.  GB/s = bytes the algorithm needs (16 n, 14 n) over that time.  `--step-ms`: the end-to-end step the per-step cost at
interval 100 is set against (bench_e2e.py: 0.652 steps/s)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    from emdr2_amd import _native
    from step_guard_bench import build, timed
    ap = argparse.ArgumentParser()
    ap.add_argument("--params", type=int, default=440388096)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--step-ms", type=float, default=1534.0)
    a = ap.parse_args()
    opt = build(a.params, False)
    gen = torch.Generator(device="cuda").manual_seed(2)
    for b in opt.buckets:                     # moments as a run leaves them
        b["m"].copy_(torch.randn(b["n"], generator=gen, device="cuda") * 1e-3)
        b["v"].copy_(torch.randn(b["n"], generator=gen, device="cuda").square() * 1e-6)
    opt.step_count = 100
    lib, sp = _native.lib(), _native.stream_ptr()
    report, keys = opt._audit_buffers()
    plans, _, _ = opt._param_stats_buffers()
    n = sum(b["n"] for b in opt.buckets)

    def audit_pass():
        for b, k in zip(opt.buckets, keys):
            _native.check(lib.emdr2_state_audit(b["master"].data_ptr(), b["m"].data_ptr(), b["v"].data_ptr(), b["work"].data_ptr(), b["n"],
                                                k.data_ptr(), report[b["idx"]].data_ptr(), sp), "state_audit")

    arms = {"param_stats": (opt.param_stats_words, 16), "state_audit": (audit_pass, 14)}
    print("# one pass over %d elements in %d buckets, %d parameters, %d items, %s"
          % (n, len(opt.buckets), len(opt.params), sum(pl["n_items"] for pl in plans), torch.cuda.get_device_name(0)))
    for fn, _ in arms.values():
        fn(); fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, (fn, _) in arms.items():
            t[k].append(timed(fn, a.inner))
    med = {k: statistics.median(v) for k, v in t.items()}
    for k, (_, per_element) in arms.items():
        print("%-12s %8.3f ms per pass (min %.3f max %.3f)  %5.2f GB  %7.1f GB/s" % (k, med[k], min(t[k]), max(t[k]), per_element * n / 1e9,
                                                                                    per_element * n / 1e6 / med[k]))
    rate = {k: per_element * n / med[k] for k, (_, per_element) in arms.items()}
    print("param_stats / state_audit: %.3f of its bytes/s, %.3f of its time" % (rate["param_stats"] / rate["state_audit"],
                                                                               med["param_stats"] / med["state_audit"]))
    whole = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.time()
        stats = opt.param_stats()
        whole.append((time.time() - t0) * 1000.0)
    assert len(stats["params"]) == len(opt.params) and sum(r["n"] for r in stats["params"].values()) == a.params
    call = statistics.median(whole)
    print("FlatAdam.param_stats() %6.3f ms by the host clock, launches, the one host read and the dict included (min %.3f max %.3f)"
          % (call, min(whole), max(whole)))
    print("at --log-param-stats-interval 100: %.4f ms per step = %.5f %% of a %.0f ms step" % (call / 100.0, call / a.step_ms, a.step_ms))


if __name__ == "__main__":
    main()
