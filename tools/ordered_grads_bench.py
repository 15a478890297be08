#!/usr/bin/env python
"""Price of --deterministic-gradients (kernels.ORDERED; include/emdr2_ops.h, "Ordered sums"), measured on the GPU in ONE process with the
two arms alternating:

  kernels   ordered against atomic at the step's shapes: dW = dy^T x for 768 x 768, 3072 x 768 and 768 x 3072 over a question group's token
            rows (the zero-fill the atomic arm needs and the workspace request of the ordered arm are inside the timed region, as they are
            in the step), the LayerNorm backward on the same rows, the reader's embedding backward (the sort of the ordered arm included)
  step      forward + backward of configs[2] at its benchmark shape, set up as tests/test_config2_gpu.py does, flag on against off on the
            same batch and parameters, and bit-equality of the gradient buckets of two steps with the flag on

    python tools/ordered_grads_bench.py [--rows 262144] [--steps 5] [--no-step] > profiles/ordered_gradients.txt

Times are device-event times around `inner` back-to-back calls, median over `rounds` alternating rounds, after a warm-up of both arms."""
import argparse
import ctypes
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def ab(name, arms, inner=10, rounds=7, note=""):
    """arms: {label: callable}; alternating rounds; prints medians and the spread of each arm"""
    for fn in arms.values():
        fn(); fn()
    torch.cuda.synchronize()
    t = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            t[k].append(timed(fn, inner))
    med = {k: statistics.median(v) for k, v in t.items()}
    cells = "  ".join("%s %8.3f ms (min %.3f max %.3f)" % (k, med[k], min(t[k]), max(t[k])) for k in arms)
    keys = list(arms)
    print("%-34s %s  %s/%s = %.3f  %s" % (name, cells, keys[1], keys[0], med[keys[1]] / med[keys[0]], note), flush=True)
    return med


def kernel_arms(rows):
    from emdr2_amd import _native
    from emdr2_amd.model import kernels as K
    lib = _native.lib()
    g = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda *s: torch.randn(s, generator=g, device="cuda").to(torch.bfloat16)

    def arm(fn, on):
        def run():
            K.ORDERED.enabled = on
            try:
                return fn()
            finally:
                K.ORDERED.enabled = False
        return run

    print("# kernels at %d token rows (one question group of configs[2], packed)" % rows)
    for N, Kd in ((768, 768), (3072, 768), (768, 3072)):
        dy, x = rnd(rows, N), rnd(rows, Kd)
        cs = torch.zeros(N, dtype=torch.float32, device="cuda")
        tiles = ((N + 255) // 256) * ((Kd + 255) // 256)
        split = max(1, min(512 // tiles, rows // 4096))
        fn = lambda: K.weight_grad_tn(dy, x, colsum=cs)
        ab("dW %d x %d (+ bias), split %d" % (N, Kd, split), {"atomic": arm(fn, False), "ordered": arm(fn, True)},
           note="slabs %.1f MB" % (split * N * Kd * 4 / 1e6))
        a, b = arm(fn, True)(), arm(fn, True)()
        c = arm(fn, False)()
        print("    two ordered calls bit-equal: %s; ordered - atomic, relative: %.2e" % (torch.equal(a, b), float((a - c).norm() / c.norm())), flush=True)
        del dy, x, a, b, c
    H = 768
    x2, dy2 = rnd(rows, H), rnd(rows, H)
    gamma, beta = torch.nn.Parameter(torch.ones(H, device="cuda")), torch.nn.Parameter(torch.zeros(H, device="cuda"))
    _, mean, rstd = K._ln_forward(x2, gamma, beta, 1e-5)

    def ln():
        gamma.grad = beta.grad = None
        return K._ln_backward(dy2, x2, gamma, beta, mean, rstd, None)
    ab("LayerNorm backward, H 768", {"atomic": arm(ln, False), "ordered": arm(ln, True)})
    del x2, dy2
    # the reader's embedding backward on the dense [sequences, 512] grid (the long list: a third of the tokens are padding, id 0)
    S, V = 512, 30624
    nseq = rows // S
    ids = torch.randint(5, 30522, (nseq, S), generator=g, device="cuda")
    lens = torch.randint(S // 4, S + 1, (nseq,), generator=g, device="cuda")
    ids = torch.where(torch.arange(S, device="cuda")[None, :] < lens[:, None], ids, torch.zeros_like(ids))
    dout = rnd(nseq * S, H) * (ids.reshape(-1, 1) != 0)
    dW, dP = torch.zeros((V, H), device="cuda"), torch.zeros((S, H), device="cuda")
    sp = _native.stream_ptr

    def emb_atomic():
        _native.check(lib.emdr2_embedding_bwd(ids.data_ptr(), None, dout.data_ptr(), dW.data_ptr(), dP.data_ptr(), None, nseq * S, S, H, 0, 0.1, 7, sp()), "emb")

    def emb_ordered():
        order = torch.sort(ids.reshape(-1), stable=True)[1]
        n = ctypes.c_size_t()
        _native.check(lib.emdr2_embedding_bwd_ordered_ws_bytes(nseq * S, nseq, S, H, 0, ctypes.byref(n)), "ws")
        ws, nws = K.ORDERED.workspace(n.value, dout.device)
        _native.check(lib.emdr2_embedding_bwd_ordered(ids.data_ptr(), None, None, nseq, order.data_ptr(), dout.data_ptr(), dW.data_ptr(), dP.data_ptr(), None,
                                                      nseq * S, S, H, 0, 0.1, 7, ws, nws, sp()), "emb ordered")
    ab("embedding backward, dense %d x %d" % (nseq, S), {"atomic": emb_atomic, "ordered": emb_ordered}, note="(sort included)")
    sort_only = lambda: torch.sort(ids.reshape(-1), stable=True)
    ab("  of which the stable sort", {"atomic": emb_atomic, "sort": sort_only})
    K.ORDERED.release()


def step_arms(steps):
    import bench_e2e
    from emdr2_amd.model import kernels as K
    from emdr2_amd.model.emdr2_model import emdr2_loss
    args = types.SimpleNamespace(batch=64, layers=12, seq=512, seq_ret=256, dropout=0.1, keep_last_layers="0", selective_layers="12,6", no_packing=False,
                                 reindex_rows_per_step=0, rows=2_000_000, micro_batches=1)
    ctx = bench_e2e.setup(args, 0, 1, topk=50)
    model, opt = ctx.model, ctx.opt
    bt = ctx.make_batch()
    model.set_recompute_keep_last(0)
    model.set_selective_retention(12, 6, 12)

    def step(on, keep=False):
        K.ORDERED.enabled = on
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        opt.zero_grad()
        lm, tlp, one = model(bt["uid"], bt["q"], bt["types"], None, bt["q"], bt["qlen"], bt["dec"])
        loss, _ = emdr2_loss(lm, tlp, one, bt["labels"], bt["mask"], eos_id=30523)
        loss.backward()
        opt.finish()
        b.record()
        torch.cuda.synchronize()
        K.ORDERED.enabled = False
        return a.elapsed_time(b), float(loss.detach()), ([x["grad"].clone() for x in opt.buckets] if keep else None)

    print("# configs[2] at its benchmark shape: B 64, top-k 50, S 512, 12 layers; forward + backward of one batch from the same parameters")
    step(False); step(True)
    t = {False: [], True: []}
    for _ in range(steps):
        for on in (False, True):
            t[on].append(step(on)[0])
    for on in (False, True):
        print("flag %-3s  %d steps: median %.1f ms (min %.1f max %.1f)" % ("on" if on else "off", steps, statistics.median(t[on]), min(t[on]), max(t[on])))
    print("on / off = %.4f" % (statistics.median(t[True]) / statistics.median(t[False])))
    _, la, ga = step(True, keep=True)
    _, lb, gb = step(True, keep=True)
    print("flag on, two steps: losses equal %s, gradient buckets bit-equal %s (%d buckets, %d elements)"
          % (la == lb, all(torch.equal(x, y) for x, y in zip(ga, gb)), len(ga), sum(x.numel() for x in ga)))
    del gb
    _, lc, gc = step(False, keep=True)
    _, ld, gd = step(False, keep=True)
    num = sum(float((x - y).double().pow(2).sum()) for x, y in zip(gc, gd)) ** 0.5
    den = sum(float(y.double().pow(2).sum()) for y in gd) ** 0.5
    print("flag off, two steps: losses equal %s, gradient buckets bit-equal %s, relative difference %.2e"
          % (lc == ld, all(torch.equal(x, y) for x, y in zip(gc, gd)), num / den))
    num = sum(float((x - y).double().pow(2).sum()) for x, y in zip(ga, gc)) ** 0.5
    print("flag on against off: losses equal %s, relative gradient difference %.2e" % (la == lc, num / den))
    print("ordered workspace: %.1f MB; peak HBM allocated %.1f GB" % (sum(w.numel() for w in K.ORDERED._ws.values()) / 1e6, torch.cuda.max_memory_allocated() / 1e9))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=262144)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("needs the GPU: nothing here is a measurement without it")
    print("# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    if not a.no_kernels:
        kernel_arms(a.rows)
    if not a.no_step:
        step_arms(a.steps)


if __name__ == "__main__":
    main()
