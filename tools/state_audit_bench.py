#!/usr/bin/env python
"""Price of one optimizer-state audit (--audit-optimizer-state-interval; FlatAdam.audit(), include/emdr2_ops.h, "State audit"), measured on
the GPU in ONE process at the benchmark's parameter count (440,388,096 elements in 512 MiB buckets): the streaming pass itself -- one
emdr2_state_audit call per bucket, 14 bytes per element -- and, alternating with it in the same run, emdr2_sumsq_f32 over the same
buckets' masters (4 bytes per element), the project's own streaming yardstick.  Then FlatAdam.audit() as the task calls it, by the host
clock: the launches plus its one host read.

    python tools/state_audit_bench.py [--params 440388096] [--rounds 9] > profiles/state_audit.txt

Kernel times are device-event times around `inner` back-to-back passes over all buckets, median over alternating rounds, after a warm-up
of both arms.  GB/s = bytes the algorithm needs (14 n, 4 n) over that time."""
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
    a = ap.parse_args()
    opt = build(a.params, False)
    gen = torch.Generator(device="cuda").manual_seed(2)
    for b in opt.buckets:                     # moments as a run leaves them (the pass is value-independent on a sound state)
        b["m"].copy_(torch.randn(b["n"], generator=gen, device="cuda") * 1e-3)
        b["v"].copy_(torch.randn(b["n"], generator=gen, device="cuda").square() * 1e-6)
    lib, sp = _native.lib(), _native.stream_ptr()
    report, keys = opt._audit_buffers()
    n = sum(b["n"] for b in opt.buckets)

    def audit_pass():
        for b, k in zip(opt.buckets, keys):
            _native.check(lib.emdr2_state_audit(b["master"].data_ptr(), b["m"].data_ptr(), b["v"].data_ptr(), b["work"].data_ptr(), b["n"],
                                                k.data_ptr(), report[b["idx"]].data_ptr(), sp), "state_audit")

    def sumsq_pass():
        for b in opt.buckets:
            _native.check(lib.emdr2_sumsq_f32(b["master"].data_ptr(), b["n"], opt._gsq.data_ptr(), opt._scratch.data_ptr(), sp), "sumsq")

    arms = {"state_audit": (audit_pass, 14), "sumsq_f32": (sumsq_pass, 4)}
    print("# one pass over %d elements in %d buckets, %s" % (n, len(opt.buckets), torch.cuda.get_device_name(0)))
    for fn, _ in arms.values():
        fn(); fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, (fn, _) in arms.items():
            t[k].append(timed(fn, a.inner))
    for k, (_, per_element) in arms.items():
        med = statistics.median(t[k])
        print("%-12s %8.3f ms per pass (min %.3f max %.3f)  %5.2f GB  %7.1f GB/s" % (k, med, min(t[k]), max(t[k]), per_element * n / 1e9,
                                                                                    per_element * n / 1e6 / med))
    whole = []
    for _ in range(a.rounds):
        torch.cuda.synchronize()
        t0 = time.time()
        res = opt.audit()
        whole.append((time.time() - t0) * 1000.0)
    assert res["sound"] and res["elements"] == n, {k: v for k, v in res.items() if k != "digests"}
    print("FlatAdam.audit() %6.3f ms by the host clock, launches and the one host read included (min %.3f max %.3f); sound, %d buckets"
          % (statistics.median(whole), min(whole), max(whole), res["buckets"]))


if __name__ == "__main__":
    main()
