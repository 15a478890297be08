"""CPU: the float64 GEMM references and majorant bounds of tests/gemm_ref.py, checked without a GPU.

  * the fp32 torch implementation of every recipe stays within every bound on every family, at or below ratio 0.5 (the ratios quoted in
    gemm_ref's docstring);
  * the GELU / GELU' absolute constants are at least twice the measured error of the fp32 Abramowitz-Stegun formula;
  * a torch model of the tiled walk of csrc/gemm.hip (K in chunks of 32, fp32 accumulation, the epilogue's order of operations and roundings,
    split-K slices of ceil(chunks / split) chunks, TN with colsum) passes every bound;
  * planted faults, one at a time, in that model: each is caught by the bounds on at least one family, and the test records which of them
    the metrics these bounds replace -- allclose(rtol 2e-2, atol 2e-2 sqrt K) and max|a - r| / max|r| < 2e-2, on randn -- let through, and which they let through even on the family that shows the fault
    (the bias at n + 1 and the overhang row's residual under smooth inputs).
"""
import math

import pytest
import torch

from tests import gemm_ref as G

M0, N0 = 80, 72

RECIPES = {                              # name -> (kwargs of the reference, outputs checked)
    "plain": (dict(), ("out",)),
    "plain_f32": (dict(out_f32=True), ("out",)),
    "bias": (dict(bias=True), ("out",)),
    "bias_alpha_f32": (dict(bias=True, alpha=0.125, out_f32=True), ("out",)),
    "gelu": (dict(bias=True, gelu=1), ("out",)),
    "gelu_f32": (dict(bias=True, gelu=1, out_f32=True), ("out",)),
    "gelu_pre": (dict(bias=True, gelu=1), ("out", "pre")),
    "gelu_der": (dict(bias=True, gelu=2), ("out", "der")),
    "radd": (dict(R=True), ("out",)),
    "bias_radd": (dict(bias=True, R=True), ("out",)),
    "bias_radd_f32": (dict(bias=True, R=True, out_f32=True), ("out",)),
    "bias_drop_radd": (dict(bias=True, R=True, drop=0.1), ("out",)),
    "rgelu": (dict(R=True, rmode=1), ("out",)),
    "rmul": (dict(R=True, rmode=2), ("out",)),
}


def _case(fam, K, recipe, seed=0, M=M0, N=N0):
    kw, outs = RECIPES[recipe]
    A, B, bias, R = G.nt_inputs(fam, M, N, K, seed)
    args = dict(alpha=kw.get("alpha", 1.0), bias=bias if kw.get("bias") else None, gelu=kw.get("gelu", 0),
                mask=G.keep_mask(M, N, kw["drop"], seed + 1) if kw.get("drop") else None, R=R if kw.get("R") else None, rmode=kw.get("rmode", 0))
    return A, B, args, bool(kw.get("out_f32")), outs


def test_gelu_formula_constants():
    x = torch.linspace(-G.GELU_GRID, G.GELU_GRID, 2_000_001, dtype=torch.float64).float()
    x = torch.cat([x, G.bf(x), torch.tensor([0.0, -0.0])])
    g, d = G.gelu_as_f32(x)
    xd = x.double()
    eg = ((g.double() - G.gelu64(xd)).abs() / xd.abs().clamp(min=1e-30))[xd != 0].max().item()
    ed = (d.double() - G.gelu_grad64(xd)).abs().max().item()
    print("GELU: max |model - float64| / |x| = %.3g (constant %.3g);  GELU': max |model - float64| = %.3g (constant %.3g)"
          % (eg, G.GELU_ABS_X, ed, G.GELUP_ABS))
    assert eg <= 0.5 * G.GELU_ABS_X and ed <= 0.5 * G.GELUP_ABS
    assert float(g[x == 0].abs().max()) == 0.0


def test_cancel_family_cancels_and_partial_sums_do_not():
    for K in (64, 256):
        A, B, _, _ = G.nt_inputs("cancel", M0, N0, K, 3)
        r = G.nt_reference(A, B)
        assert float((r.pre.abs() * 1024.0 / r.S).max()) <= 1.0
        half = G.nt_reference(A[:, :K // 2], B[:, :K // 2])
        assert float((half.pre.abs() / half.S).median()) > 0.05
    A, B = G.tn_inputs("cancel", 96, 40, 48, 3)
    t = G.tn_reference(A, B)
    assert float((t.dW.abs() * 1024.0 / t.S).max()) <= 1.0


@pytest.mark.parametrize("recipe", sorted(RECIPES))
def test_fp32_torch_reference_within_half_of_every_bound(recipe):
    worst = {}
    for fam in G.FAMILIES:
        for K in (64, 768):
            A, B, args, f32, outs = _case(fam, K, recipe, seed=K)
            r = G.nt_reference(A, B, **args)
            bd = G.nt_bounds(r, out_f32=f32)
            got = G.nt_torch_f32(A, B, out_f32=f32, **args)
            for o in outs:
                ratio, idx = G.worst(got[o], getattr(r, o), bd[o])
                worst[o] = max(worst.get(o, 0.0), ratio)
                assert ratio <= 0.5, (recipe, fam, K, o, ratio, idx)
    print("fp32 torch reference, %-16s %s" % (recipe, "  ".join("%s %.2f" % kv for kv in sorted(worst.items()))))


def test_fp32_torch_reference_exact_families():
    for K in (64, 768):
        for f32 in (False, True):
            for fam in G.EXACT_FAMILIES:
                A, B, bias, _ = G.nt_inputs(fam, 800, N0, K, 0, f32_codes=f32)
                got = G.nt_torch_f32(A, B, bias=bias, out_f32=f32)["out"]
                assert torch.equal(got, G.nt_exact(fam, 800, N0, K, f32_codes=f32)), (fam, K, f32)
                assert torch.equal(G.nt_reference(A, B, bias=bias).out.float(), got)
                if fam == "onehot_k":
                    assert bool((A.sum(0) >= 1).all())                   # M >= K: every k position is read


def test_fp32_torch_reference_tn_and_lse():
    worst = {}
    for fam in G.FAMILIES + ("onehot_k",):
        for R in (96, 2080):
            A, B = G.tn_inputs(fam, R, 40, 72, R)
            r = G.tn_reference(A, B)
            bd, got = G.tn_bounds(r), G.tn_torch_f32(A, B)
            for o in ("dW", "colsum"):
                ratio, idx = G.worst(got[o], getattr(r, o), bd[o])
                worst[o] = max(worst.get(o, 0.0), ratio)
                assert ratio <= 0.5, (fam, R, o, ratio, idx)
            if fam == "onehot_k":
                assert torch.equal(got["dW"], B[(37 * torch.arange(40) + 5) % R]) and torch.equal(got["colsum"], torch.ones(40))
    for fam in ("row_scaled", "smooth"):
        A, B, bias, labels = G.lse_inputs(fam, 48, 256, 128, 5)
        r = G.lse_nt_reference(A, B, 1.0, bias, labels)
        assert float(r.logits.abs().max()) > 200.0
        ratio, idx = G.worst(G.lse_torch_f32(A, B, 1.0, bias, labels)["gold"], r.gold, G.lse_nt_bounds(r)["gold"])
        worst["gold"] = max(worst.get("gold", 0.0), ratio)
        assert ratio <= 0.5, (fam, ratio, idx)
        out = torch.tensor([1, 3, 5])
        assert torch.equal(r.gold[out], -r.L.lse[out])
    print("fp32 torch reference, TN / LSE   %s" % "  ".join("%s %.2f" % kv for kv in sorted(worst.items())))


# ---- the tiled walk of csrc/gemm.hip as a torch model, with planted faults --------------------------------------------------------------
def model_nt(A, B, alpha=1.0, bias=None, gelu=0, mask=None, R=None, rmode=0, out_f32=False, split=1, fault=None):
    """K in chunks of 32 with an fp32 accumulator; slices of per = ceil(chunks / split) chunks summed in fp32 (the atomics); then the epilogue
    in the kernel's order: acc * alpha + bias -> second output (bf16) -> GELU -> dropout -> bf16 -> residual -> store."""
    a, b = A.float(), B.float()
    if fault == "fp16_operands":                                         # the operands taken through the wrong 16-bit format
        a, b = a.half().float(), b.half().float()
    if fault == "swap_groups":                                           # two 16-byte groups of one K chunk swapped between rows 0 and 1
        a = a.clone()
        a[0, 40:48], a[1, 40:48] = A[1, 40:48].float(), A[0, 40:48].float()
    M, K = a.shape
    N = b.shape[0]
    chunks = K // 32
    per = -(-chunks // split)
    slices = [(z * per, min(per, max(chunks - z * per, 0))) for z in range(split)]
    last = max(z for z, (_, n) in enumerate(slices) if n > 0)
    total = torch.zeros((M, N))
    for z, (c0, n) in enumerate(slices):
        if n == 0:
            continue
        acc = torch.zeros((M, N))
        for c in range(c0, c0 + n):
            part = a[:, 32 * c:32 * c + 32] @ b[:, 32 * c:32 * c + 32].t()
            if fault == "drop_last_chunk" and c == chunks - 1:
                part[16:32] = 0.0                                        # the rows of one 16-row piece
            acc = acc + part
            if fault == "round_mid_k" and c == chunks // 2 - 1:
                acc = G.bf(acc)
            if fault == "bf16_accumulator":
                acc = G.bf(acc)
        total = total + acc
        if fault == "slice_twice" and z == last and chunks % split:
            total = total + acc
    bv = torch.zeros(N) if bias is None else bias.float()
    if fault == "bias_n_plus_1":
        bv = torch.cat([bv[1:], bv[-1:]])                                # (the last column re-reads itself)
    if fault == "bias_bf16":
        bv = G.bf(bv)
    v = (total + bv) * alpha if fault == "alpha_after_bias" else total * alpha + bv
    got = {"pre": G.bf(v)}
    if gelu:
        v, d = G.gelu_as_f32(v)
        if gelu == 2:
            got["der"] = G.bf(d)
    rnd = (lambda t: t) if out_f32 else G.bf
    Rf = None if R is None else R.float()
    if fault == "residual_row_above":                                    # an overhang row's epilogue lands in row M - 1: the accumulator is that of the
        # clamped row M - 1 itself, what differs is the row the residual is read at (the row above stands in for it)
        # -- a gentle stand-in (1.5 % between smooth rows); an ACCUMULATOR from a wrong row is what onehot_k and coded catch, exactly
        Rf = Rf.clone()
        Rf[M - 1] = Rf[M - 2]
    if fault == "residual_before_mask":
        v = (rnd(v) + Rf) * mask.float()
    else:
        if mask is not None:
            v = v * mask.float()
        if Rf is not None:
            v = rnd(v)
            v = v + Rf if rmode == 0 else (v * Rf if rmode == 2 else v * G.gelu_as_f32(Rf)[1])
    got["out"] = rnd(v)
    return got


def model_tn(A, B, split=1, fault=None):
    a, b = A.float(), B.float()
    R, I = a.shape
    chunks = R // 32
    per = -(-chunks // split)
    dW, col = torch.zeros((I, b.shape[1])), torch.zeros(I)
    for z in range(split):
        c0, n = z * per, min(per, max(chunks - z * per, 0))
        acc, cs = torch.zeros_like(dW), torch.zeros(I)
        for c in range(c0, c0 + n):
            acc = acc + a[32 * c:32 * c + 32].t() @ b[32 * c:32 * c + 32]
            cs = cs + a[32 * c:32 * c + 32].sum(0)
        if fault == "colsum_granule_twice":                              # the clamped overhang granule re-reads columns I - 8 .. I - 1
            cs[I - 8:] = cs[I - 8:] * 2.0
        dW, col = dW + acc, col + cs
    return {"dW": dW, "colsum": col}


@pytest.mark.parametrize("recipe", sorted(RECIPES))
def test_faithful_model_passes_every_bound(recipe):
    for fam in G.FAMILIES:
        for K, split in ((64, 1), (160, 4), (768, 1)):                    # 160: chunks = 5, split = 4: slices of 2, 2, 1 and an empty one
            if split > 1 and recipe != "plain_f32":
                continue
            A, B, args, f32, outs = _case(fam, K, recipe, seed=K + 1)
            r = G.nt_reference(A, B, **args)
            bd = G.nt_bounds(r, out_f32=f32, slices=split)
            got = model_nt(A, B, out_f32=f32, split=split, **args)
            for o in outs:
                ratio, idx = G.worst(got[o], getattr(r, o), bd[o])
                assert ratio <= 1.0, (recipe, fam, K, split, o, ratio, idx)


def test_faithful_model_exact_families_tn_and_lse():
    for fam in G.EXACT_FAMILIES:
        for f32 in (False, True):
            A, B, bias, _ = G.nt_inputs(fam, 800, N0, 160, 0, f32_codes=f32)
            got = model_nt(A, B, bias=bias, out_f32=f32, split=4 if f32 and bias is None else 1)["out"]
            assert torch.equal(got, G.nt_exact(fam, 800, N0, 160, f32_codes=f32)), (fam, f32)
    for fam in G.FAMILIES + ("onehot_k",):
        for R, split in ((96, 1), (2080, 7)):
            A, B = G.tn_inputs(fam, R, 40, 72, R + 1)
            r, got = G.tn_reference(A, B), model_tn(A, B, split)
            bd = G.tn_bounds(r, split)
            for o in ("dW", "colsum"):
                ratio, idx = G.worst(got[o], getattr(r, o), bd[o])
                assert ratio <= 1.0, (fam, R, o, ratio, idx)


# fault -> (family that must catch it, K, recipe, output, split)
FAULTS = {
    "drop_last_chunk": ("row_scaled", 256, "plain", "out", 1),
    "round_mid_k": ("cancel", 256, "plain", "out", 1),
    "bf16_accumulator": ("cancel", 256, "bias", "out", 1),
    "fp16_operands": ("row_scaled", 256, "plain", "out", 1),
    "bias_n_plus_1": ("smooth", 256, "bias", "out", 1),
    "bias_bf16": ("smooth", 256, "bias_alpha_f32", "out", 1),
    "alpha_after_bias": ("cancel", 256, "bias_alpha_f32", "out", 1),
    "residual_before_mask": ("smooth", 256, "bias_drop_radd", "out", 1),
    "residual_row_above": ("smooth", 256, "bias_radd_f32", "out", 1),
    "slice_twice": ("randn", 160, "plain_f32", "out", 4),
    "swap_groups": ("onehot_k", 64, "plain", "out", 1),
}
# the old metrics on randn let these through; fp16_operands (exact on randn's range) and bias_bf16 (one 2^-9 rounding of the bias) are
# near no-ops there, the first two are the substantive ones
OLD_METRICS_MUST_PASS = ("round_mid_k", "bf16_accumulator", "fp16_operands", "bias_bf16")
# ... and these they let through on the very family that shows the fault: the old metrics do not become sharper on better inputs
OLD_METRICS_MUST_PASS_ON_THE_FAMILY = ("bias_n_plus_1", "residual_row_above", "bias_bf16")


def _old_metrics_pass(got, ref, K):
    return bool(torch.allclose(got.float(), ref.float(), rtol=2e-2, atol=2e-2 * math.sqrt(K))) and G.old_metric(got, ref) < 2e-2


def test_planted_faults_are_caught_and_which_the_old_metrics_let_through():
    caught, old_pass, old_pass_fam = {}, {}, {}
    for fault, (fam, K, recipe, o, split) in sorted(FAULTS.items()):
        if fam == "onehot_k":
            A, B, bias, _ = G.nt_inputs(fam, M0, N0, K, 0)
            caught[fault] = not torch.equal(model_nt(A, B, bias=bias, fault=fault)["out"], G.nt_exact(fam, M0, N0, K))
            assert torch.equal(model_nt(A, B, bias=bias)["out"], G.nt_exact(fam, M0, N0, K))
        else:
            A, B, args, f32, _ = _case(fam, K, recipe, seed=11)
            r = G.nt_reference(A, B, **args)
            got = model_nt(A, B, out_f32=f32, split=split, fault=fault, **args)[o]
            ratio, _ = G.worst(got, getattr(r, o), G.nt_bounds(r, out_f32=f32, slices=split)[o])
            caught[fault] = ratio > 1.0
            old_pass_fam[fault] = _old_metrics_pass(got, getattr(r, o), K)
        A, B, args, f32, _ = _case("randn", K, recipe, seed=12)           # the old metrics, on randn
        r = G.nt_reference(A, B, **args)
        old_pass[fault] = _old_metrics_pass(model_nt(A, B, out_f32=f32, split=split, fault=fault, **args)[o], getattr(r, o), K)
    # TN: the colsum's overhang granule counted twice
    A, B = G.tn_inputs("row_scaled", 96, 40, 72, 2)
    r = G.tn_reference(A, B)
    caught["colsum_granule_twice"] = G.worst(model_tn(A, B, fault="colsum_granule_twice")["colsum"], r.colsum, G.tn_bounds(r)["colsum"])[0] > 1.0
    A, B = G.tn_inputs("randn", 96, 40, 72, 2)
    old_pass["colsum_granule_twice"] = _old_metrics_pass(model_tn(A, B, fault="colsum_granule_twice")["colsum"], G.tn_reference(A, B).colsum, 96)
    # LSE: the gold logit picked from the neighbouring 64-column wave slice
    for fam, store in (("smooth", caught), ("row_scaled", old_pass)):
        A, B, bias, labels = G.lse_inputs(fam, 48, 256, 128, 5)
        r = G.lse_nt_reference(A, B, 1.0, bias, labels)
        got = G.lse_torch_f32(A, B, 1.0, bias, torch.where(r.L.inside, (labels + 64) % 256, labels))["gold"]
        if store is caught:
            caught["lse_neighbour_slice"] = G.worst(got, r.gold, G.lse_nt_bounds(r)["gold"])[0] > 1.0
        else:
            old_pass["lse_neighbour_slice"] = bool(torch.allclose(got, r.gold.float(), rtol=2e-2, atol=5e-2))
    for f in sorted(caught):
        print("fault %-24s caught by the bounds: %-5s  passes the old metrics on randn: %-5s  on the catching family: %s"
              % (f, caught[f], old_pass[f], old_pass_fam.get(f, "-")))
    assert len(caught) >= 8 and all(caught.values()), caught
    assert all(old_pass[f] for f in OLD_METRICS_MUST_PASS), old_pass
    assert sum(old_pass.values()) >= 4
    assert all(old_pass_fam[f] for f in OLD_METRICS_MUST_PASS_ON_THE_FAMILY), old_pass_fam
