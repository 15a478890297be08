"""tests/elementwise_ref.py checked on the CPU: (1) its float64 references agree with torch autograd in float64; (2) the fp32 torch
implementation of every op stays within every bound on every input family the GPU tests use (the check that inputs and bounds are
compatible, and the measurement behind the constants recorded in elementwise_ref.py: run with -s to see the ratios); (3) planted faults
that the whole-tensor metric max|a - r| / max|r| < 2e-2 accepts are rejected by the bounds."""
import math

import pytest
import torch

from tests import elementwise_ref as R

OLD_TOL = 2e-2
EPS = 1e-5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _close64(a, b, tol=1e-10):
    scale = float(b.abs().max()) + 1e-300
    assert float((a - b).abs().max()) <= tol * max(scale, 1.0), (float((a - b).abs().max()), scale)


def _report(tag, ratios, limit=0.5):
    print("[ew-ref] %s " % tag + " ".join("%s=%.3f" % (n, r[0]) for n, r in ratios.items()))
    bad = {n: r for n, r in ratios.items() if not r[0] <= limit}
    assert not bad, (tag, bad)


# ---- (1) the references against autograd in float64 -----------------------------------------------------------------------------------
def test_layernorm_reference_is_autograd_in_float64():
    x, gamma, beta, dy, dres = [t.double() for t in R.ln_inputs("offset8", "randn", 9, 264, _gen(1))]
    r = R.ln_reference(x, gamma, beta, EPS, dy, dres)
    xx, g, b = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xx, (264,), g, b, EPS)
    (y * dy).sum().backward()
    _close64(r.y, y.detach())
    _close64(r.dx, xx.grad + dres)
    _close64(r.dgamma, g.grad)
    _close64(r.dbeta, b.grad)
    _close64(r.mean, x.mean(-1))
    _close64(r.rstd, (x.var(-1, unbiased=False) + EPS).rsqrt())


def test_lse_gather_reference_is_autograd_in_float64():
    x, labels, w = R.lse_inputs("dominant", 5, 257, _gen(2))
    labels[2], labels[3] = -100, 257 + 7
    w[2] = 0.75
    r = R.lse_reference(x, labels, w)
    xx = x.double().requires_grad_(True)
    lp = torch.log_softmax(xx, -1)
    inside = (labels >= 0) & (labels < 257)
    gold = torch.where(inside, lp.gather(1, labels.clamp(0, 256)[:, None])[:, 0], -torch.logsumexp(xx, -1))
    (gold * w.double()).sum().backward()
    _close64(r.gold, gold.detach())
    _close64(r.dlogits, xx.grad)
    _close64(r.dlogits[2], -w[2].double() * torch.softmax(x[2].double(), -1))            # an ignored row: -w softmax


def test_combine_reference_is_logsumexp_of_the_slots():
    pmax, psum, gold = R.combine_inputs(7, 65, _gen(3))
    r = R.combine_reference(pmax, psum, gold)
    _close64(r.lse, torch.logsumexp(pmax.double() + psum.double().log(), -1))
    _close64(r.out, gold.double() - r.lse)


def test_prior_and_marginal_references_are_autograd_in_float64():
    q, c, scale, g = R.prior_inputs("wide", 3, 7, 264, _gen(4))
    r = R.prior_reference(q, c, scale, g)
    qq, cc = q.double().requires_grad_(True), c.double().requires_grad_(True)
    logp = torch.log_softmax(torch.einsum("bh,bkh->bk", qq, cc) * scale, -1)
    (logp * g.double()).sum().backward()
    _close64(r.logp, logp.detach())
    _close64(r.dq, qq.grad)
    _close64(r.dc, cc.grad)
    prior, gold, gm = R.marginal_inputs(3, 51, 65, _gen(5))
    rm = R.marginal_reference(prior, gold, gm)
    p = prior.double().requires_grad_(True)
    out = torch.logsumexp(p[:, :, None] + gold.double(), 1)
    (out * gm.double()).sum().backward()
    _close64(rm.marginal, out.detach())
    _close64(rm.dprior, p.grad)
    _close64(rm.dprior.sum(-1), gm.double().sum(-1), 1e-9)


def test_gelu_reference_is_autograd_in_float64():
    x, dact = R.gelu_inputs(264, _gen(6))
    r = R.gelu_bwd_reference(x, dact)
    xx = x.double().requires_grad_(True)
    (torch.nn.functional.gelu(xx) * dact.double()).sum().backward()
    assert float((r.dpre - xx.grad).abs().max()) < 1e-15 * 10


def test_adam_reference_is_torch_adamw_in_float64():
    # hyper-parameters that fp32 holds exactly, so that the rounding adam_reference applies to them changes nothing
    lr, b1, b2, eps, wd, clip = 2.0 ** -7, 0.875, 1.0 - 2.0 ** -10, 2.0 ** -27, 0.125, 0.5
    g = _gen(7)
    w = torch.randn(1028, generator=g, dtype=torch.float64)
    p = torch.nn.Parameter(w.clone())
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    m, v, cur = torch.zeros_like(w), torch.zeros_like(w), w.clone()
    for step in (1, 2, 3):
        grad = torch.randn(1028, generator=g, dtype=torch.float64) * (3.0 if step != 2 else 1e-3)    # step 2: norm < clip, no scaling
        p.grad = grad.clone()
        torch.nn.utils.clip_grad_norm_([p], clip)
        opt.step()
        r = R.adam_reference(cur, grad, m, v, lr, b1, b2, eps, wd, step, float((grad ** 2).sum()), clip)
        assert (r.scale < 1.0) == (step != 2)
        _close64(r.master, p.detach(), 1e-6)         # the host's fp32 bias corrections against torch's float64 ones
        _close64(r.m, opt.state[p]["exp_avg"], 1e-6)
        _close64(r.v, opt.state[p]["exp_avg_sq"], 1e-6)
        cur, m, v = p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()


# ---- (2) the fp32 torch implementation within every bound on every family --------------------------------------------------------------
@pytest.mark.parametrize("H", [8, 264, 768, 1024])
@pytest.mark.parametrize("fam", R.LN_X_FAMILIES)
def test_torch_f32_layernorm_within_bounds(fam, H):
    for dyfam in R.LN_DY_FAMILIES:
        x, gamma, beta, dy, dres = R.ln_inputs(fam, dyfam, 33, H, _gen(H + len(fam)))
        ref = R.ln_reference(x, gamma, beta, EPS, dy, dres)
        _report("ln %s %s H=%d" % (fam, dyfam, H), R.worst_all(R.ln_torch_f32(x, gamma, beta, EPS, dy, dres), ref, R.ln_bounds(ref)))


@pytest.mark.parametrize("fam", ["randn", "offset200", "outlier256"])
def test_torch_f32_layernorm_within_bounds_two_laps(fam):
    x, gamma, beta, dy, dres = R.ln_inputs(fam, "randn", 16393, 768, _gen(9))
    ref = R.ln_reference(x, gamma, beta, EPS, dy, dres)
    _report("ln %s rows=16393" % fam, R.worst_all(R.ln_torch_f32(x, gamma, beta, EPS, dy, dres), ref, R.ln_bounds(ref)))


# fp32 constants (the validation path, tests/test_fp32_path_edges_gpu.py): c = C_F32, mant_bits = 23, mean_terms = True.  Two fp32
# implementations are held to them: the formula as csrc/fp32_ops.hip states it (every family, every quantity), and dx of torch's own
# fp32 layer_norm on the families whose |mean| / std is at most 8 or whose rows are constant.  torch's backward forms dx from x, not
# from x - mean, so its error grows with that ratio, and its forward has a variance algorithm of its own (y up to 1.5 bounds, dgamma
# 1.4): what it scores elsewhere is printed, not asserted -- it is no reference there.
LN_TORCH_F32_FAMILIES = ("randn", "offset8", "const0", "const1", "const256", "alternating", "tiny")


@pytest.mark.parametrize("rows", [1, 5, 1031])
@pytest.mark.parametrize("H", [8, 63, 264, 768])
def test_fp32_layernorm_within_the_fp32_bounds(H, rows):
    worst_formula, worst_torch, worst_other = {}, {}, {}
    for fam in R.LN_X_FAMILIES:
        for dyfam in R.LN_DY_FAMILIES:
            x, gamma, beta, dy, dres = R.ln_inputs(fam, dyfam, rows, H, _gen(rows * 7 + H))
            for dr in (None, dres):
                ref = R.ln_reference(x, gamma, beta, EPS, dy, dr)
                B = R.ln_bounds(ref, R.C_F32, 23, mean_terms=True)
                pairs = [(worst_formula, R.ln_formula_f32(x, gamma, beta, EPS, dy, dr)),
                         (worst_torch if fam in LN_TORCH_F32_FAMILIES else worst_other, R.ln_torch_f32(x, gamma, beta, EPS, dy, dr, store_bf16=False))]
                for into, got in pairs:
                    for n, v in R.worst_all(got, ref, B).items():
                        if v[0] > into.get(n, (-1.0,))[0]:
                            into[n] = v
    print("[ew-ref] fp32 ln rows=%d H=%d torch outside its families (not asserted): " % (rows, H) + " ".join("%s=%.2f" % (n, r[0]) for n, r in worst_other.items()))
    _report("fp32 ln rows=%d H=%d formula" % (rows, H), worst_formula)
    print("[ew-ref] fp32 ln rows=%d H=%d torch on its families (dx asserted): " % (rows, H) + " ".join("%s=%.2f" % (n, r[0]) for n, r in worst_torch.items()))
    _report("fp32 ln rows=%d H=%d torch" % (rows, H), {"dx": worst_torch["dx"]})


@pytest.mark.parametrize("fam,H", [("const0", 768), ("tiny", 768), ("const0", 8)])
def test_dx_bound_by_the_values_of_its_means_cannot_be_met_in_fp32(fam, H):
    """ln_bounds without mean_terms at the fp32 constant: m1 = mean_j g_j cancels on some of 1,031 rows, and both fp32 implementations miss
    c rstd |m1| there while they stay within half the bound that weighs the mean by mean |g|."""
    worst = {"formula": 0.0, "torch": 0.0, "formula_terms": 0.0, "torch_terms": 0.0}
    for dyfam in R.LN_DY_FAMILIES:
        x, gamma, beta, dy, dres = R.ln_inputs(fam, dyfam, 1031, H, _gen(1031 * 7 + H))
        ref = R.ln_reference(x, gamma, beta, EPS, dy, dres)
        by_value, by_terms = R.ln_bounds(ref, R.C_F32, 23)["dx"], R.ln_bounds(ref, R.C_F32, 23, mean_terms=True)["dx"]
        for name, got in (("formula", R.ln_formula_f32(x, gamma, beta, EPS, dy, dres)), ("torch", R.ln_torch_f32(x, gamma, beta, EPS, dy, dres, store_bf16=False))):
            worst[name] = max(worst[name], R.worst(got["dx"], ref.dx, by_value)[0])
            worst[name + "_terms"] = max(worst[name + "_terms"], R.worst(got["dx"], ref.dx, by_terms)[0])
    print("[ew-ref] fp32 dx %s H=%d: by value formula %.1f torch %.1f; by terms formula %.2f torch %.2f"
          % (fam, H, worst["formula"], worst["torch"], worst["formula_terms"], worst["torch_terms"]))
    assert worst["formula"] > 1.0 and worst["torch"] > 1.0
    assert worst["formula_terms"] <= 0.5 and worst["torch_terms"] <= 0.5


def test_recursive_fp32_column_sum_of_1031_like_rows_needs_the_recursive_constant():
    """dgamma of `alternating` rows with a constant dy at H = 63: the terms of a column are all alike.  Summed row by row in fp32 (what one
    atomic per row does) the sum leaves C_F32's bound and stays within half of max(C_F32, (rows + 2) U32); torch's pairwise sum stays
    within C_F32's."""
    rows, H = 1031, 63
    x, gamma, beta, dy, dres = R.ln_inputs("alternating", "const", rows, H, _gen(rows * 7 + H))
    ref = R.ln_reference(x, gamma, beta, EPS, dy, None)
    got = R.ln_formula_f32(x, gamma, beta, EPS, dy, None)
    terms = dy.float() * ((x.float() - got["mean"][:, None]) * got["rstd"][:, None])
    acc = torch.zeros(H)
    for i in range(rows):
        acc = acc + terms[i]
    tree, rec = R.ln_bounds(ref, R.C_F32, 23, mean_terms=True)["dgamma"], R.ln_bounds(ref, R.C_F32, 23, mean_terms=True, recursive_rows=rows)["dgamma"]
    ratios = {"recursive/C_F32": R.worst(acc, ref.dgamma, tree), "recursive/recursive": R.worst(acc, ref.dgamma, rec), "pairwise/C_F32": R.worst(got["dgamma"], ref.dgamma, tree)}
    print("[ew-ref] fp32 dgamma alternating/const 1031 x 63: " + " ".join("%s=%.3f" % (n, r[0]) for n, r in ratios.items()))
    assert ratios["recursive/C_F32"][0] > 1.0 and ratios["recursive/recursive"][0] <= 0.5 and ratios["pairwise/C_F32"][0] <= 0.5


LSE_CASES = [(fam, V, rows, False) for fam in R.LSE_FAMILIES for V in (1, 7, 255, 257, 1000) for rows in (1, 5)] + \
            [(fam, V, 5, True) for fam in R.LSE_FAMILIES for V in (255, 257, 1000)]


def test_lse_inputs_reach_every_label_the_kernels_can_get_wrong():
    for V in (255, 257, 1000):
        _, labels, w = R.lse_inputs("randn", 5, V, _gen(V))
        assert labels.tolist()[:4] == [0, V - 1, min(255, V - 1), min(256, V - 1)] and (V <= 256 or int(labels[4]) > 255)
        assert float(w[0]) == 0.0 and float(w[1]) < 0.0 and float(w[1:].abs().min()) >= 0.25
        _, labels, w = R.lse_inputs("randn", 5, V, _gen(V), out_of_range=True)
        assert labels.tolist()[1] == -100 and labels.tolist()[3] == V + 7 and float(w[3].abs()) >= 0.25
        _, labels, w = R.lse_inputs("randn", 1, V, _gen(V))
        assert labels.tolist() == [V - 1] and float(w.abs().min()) >= 0.25


@pytest.mark.parametrize("store_bf16", [True, False])
@pytest.mark.parametrize("fam,V,rows,out_of_range", LSE_CASES)
def test_torch_f32_lse_gather_within_bounds(fam, V, rows, out_of_range, store_bf16):
    x, labels, w = R.lse_inputs(fam, rows, V, _gen(V + rows), out_of_range=out_of_range)
    ref = R.lse_reference(x, labels, w)
    c, mb = (R.C_BF16, 7) if store_bf16 else (R.C_F32, 23)
    _report("lse %s V=%d rows=%d out=%d bf16=%d" % (fam, V, rows, out_of_range, store_bf16),
            R.worst_all(R.lse_torch_f32(x, labels, w, store_bf16), ref, R.lse_bounds(ref, c, mb)))


@pytest.mark.parametrize("slots", [1, 3, 64, 65, 480])
def test_torch_f32_combine_within_bounds(slots):
    pmax, psum, gold = R.combine_inputs(9, slots, _gen(slots))
    ref = R.combine_reference(pmax, psum, gold)
    lse = torch.logsumexp(pmax + psum.log(), -1)
    _report("combine slots=%d" % slots, R.worst_all({"lse": lse, "out": gold - lse}, ref, R.combine_bounds(ref)))


@pytest.mark.parametrize("shape", [(2, 1, 8), (3, 7, 264), (2, 1024, 64), (2, 101, 768)])
@pytest.mark.parametrize("fam", R.PRIOR_FAMILIES)
def test_torch_f32_prior_within_bounds(fam, shape):
    q, c, scale, g = R.prior_inputs(fam, *shape, gen=_gen(shape[1]))
    ref = R.prior_reference(q, c, scale, g)
    _report("prior %s %s" % (fam, shape), R.worst_all(R.prior_torch_f32(q, c, scale, g), ref, R.prior_bounds(ref)))


@pytest.mark.parametrize("shape", [(2, 1, 1), (3, 51, 65), (2, 101, 32)])
def test_torch_f32_marginal_within_bounds(shape):
    prior, gold, gm = R.marginal_inputs(*shape, gen=_gen(shape[1]))
    assert shape[1] == 1 or float(prior.min()) < -300.0
    ref = R.marginal_reference(prior, gold, gm)
    got = R.marginal_torch_f32(prior, gold, gm)
    B = R.marginal_bounds(ref)
    ratios = R.worst_all(got, ref, {"marginal": B["marginal"], "dprior": B["dprior"]})
    ratios["identity"] = R.worst(got["dprior"].double().sum(-1), gm.double().sum(-1), B["identity"])
    _report("marginal %s" % (shape,), ratios)


def test_gelu_formula_error():
    """The absolute error of the derivative as the kernel states it, evaluated in fp32: GELU_ABS is twice the measured maximum."""
    x, dact = R.gelu_inputs(65544, _gen(11))
    ref = R.gelu_bwd_reference(x, torch.ones_like(x))
    err = float((R.gelu_formula_f32(x).double() - ref.dpre).abs().max())
    print("[ew-ref] gelu formula in fp32: max abs error %.3g, GELU_ABS %.3g" % (err, R.GELU_ABS))
    assert err <= 0.5 * R.GELU_ABS
    ref = R.gelu_bwd_reference(x, dact)
    got = R.bf(dact * R.gelu_formula_f32(x))
    _report("gelu_bwd", R.worst_all({"dpre": got}, ref, R.gelu_bwd_bounds(ref)))


@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_torch_f32_adamw_within_bounds(wd):
    # betas that fp32 holds exactly: the kernel forms 1 - beta from the fp32 beta (as apex FusedAdam does), torch rounds the float64
    # 1 - beta; at beta2 = 0.999 the two differ by 1.3e-5 of v, a convention and no rounding error.  adam_reference follows the kernel.
    lr, b1, b2, eps, clip = 1e-3, 0.90625, 1.0 - 2.0 ** -10, 1e-8, 1.0
    g = _gen(12)
    p = torch.nn.Parameter(torch.randn(1028, generator=g))
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    m, v = torch.zeros(1028), torch.zeros(1028)
    for step in (1, 2, 3):
        grad = torch.randn(1028, generator=g) * (3.0 if step != 2 else 1e-3)
        cur = p.detach().clone()
        p.grad = grad.clone()
        gsq = float((grad.double() ** 2).sum())
        torch.nn.utils.clip_grad_norm_([p], clip)
        opt.step()
        ref = R.adam_reference(cur, grad, m, v, lr, b1, b2, eps, wd, step, gsq, clip)
        got = {"master": p.detach(), "m": opt.state[p]["exp_avg"], "v": opt.state[p]["exp_avg_sq"]}
        _report("adamw wd=%g step %d" % (wd, step), R.worst_all(got, ref, R.adam_bounds(ref)))
        m, v = got["m"].clone(), got["v"].clone()


@pytest.mark.parametrize("fam", ["randn", "wide", "zero"])
def test_torch_f32_sumsq_within_bounds(fam):
    g = _sumsq_data(fam, 2097153, _gen(13))
    s, bound = R.sumsq_bound(g)
    ratio = float((float((g * g).sum()) - s).abs() / bound)
    print("[ew-ref] sumsq %s ratio %.3f" % (fam, ratio))
    assert ratio <= 0.5


def _sumsq_data(fam, n, gen):
    if fam == "randn":
        return torch.randn(n, generator=gen)
    if fam == "wide":                                                    # magnitudes from 1e-12 to 1e6
        return torch.randn(n, generator=gen).sign() * 10.0 ** (-12.0 + 18.0 * torch.rand(n, generator=gen))
    return torch.zeros(n)


# ---- (3) planted faults: accepted by the whole-tensor metric, rejected by the bounds ---------------------------------------------------
@pytest.mark.parametrize("fam", ["offset64", "offset200"])
def test_one_pass_fp32_variance_is_caught(fam):
    x, gamma, beta, dy, dres = R.ln_inputs(fam, "randn", 33, 768, _gen(21))
    ref = R.ln_reference(x, gamma, beta, EPS, dy, dres)
    mu = x.sum(-1) / 768.0
    var = ((x * x).sum(-1) / 768.0 - mu * mu).clamp_min(0.0)             # E[x^2] - mu^2 in fp32
    rstd = torch.rsqrt(var + EPS)
    y = R.bf((x - mu[:, None]) * rstd[:, None] * gamma + beta)
    B = R.ln_bounds(ref)
    assert R.old_metric(y, ref.y) < OLD_TOL and R.old_metric(rstd, ref.rstd) < OLD_TOL
    assert R.worst(rstd, ref.rstd, B["rstd"])[0] > 1.0
    # ... while the centred form in the same fp32 passes
    xc = x - mu[:, None]
    good = torch.rsqrt((xc * xc).sum(-1) / 768.0 + EPS)
    assert R.worst(good, ref.rstd, B["rstd"])[0] < 0.5


def test_row_dropped_from_dgamma_on_the_second_lap_is_caught():
    x, gamma, beta, dy, dres = R.ln_inputs("randn", "randn", 16393, 768, _gen(22))
    ref = R.ln_reference(x, gamma, beta, EPS, dy, dres)
    bad = ref.dgamma - ref.dy[16390] * ref.xhat[16390]                   # a row of the tail on lap two
    assert R.old_metric(bad, ref.dgamma) < OLD_TOL
    assert R.worst(bad, ref.dgamma, R.ln_bounds(ref)["dgamma"])[0] > 1.0


def test_gold_from_the_neighbouring_row_is_caught():
    x, labels, w = R.lse_inputs("staircase", 5, 1000, _gen(23))
    ref = R.lse_reference(x, labels, w)
    nb = torch.roll(ref.x, -1, 0)
    bad = nb.gather(1, labels[:, None])[:, 0] - ref.lse
    assert float((bad - ref.gold).abs().max()) > 0
    assert R.old_metric(bad, ref.gold) < OLD_TOL
    assert R.worst(bad, ref.gold, R.lse_bounds(ref)["gold"])[0] > 1.0


def test_block_max_not_subtracted_in_one_slot_is_caught():
    pmax, psum, gold = R.combine_inputs(64, 480, _gen(24))
    ref = R.combine_reference(pmax, psum, gold)
    pm, ps = pmax.double(), psum.double()
    wgt = torch.exp(pm - ref.m[:, None])
    wgt[:, 7] = 1.0                                                      # slot 7 added as if its maximum were the row's
    bad = gold.double() - (ref.m + torch.log((ps * wgt).sum(-1)))
    assert R.old_metric(bad, ref.out) < OLD_TOL
    assert R.worst(bad, ref.out, R.combine_bounds(ref)["out"])[0] > 1.0


def test_weight_decay_past_the_split_is_caught():
    g = _gen(25)
    w, grad = torch.randn(1028, generator=g), torch.randn(1028, generator=g)
    m, v = torch.zeros(1028), torch.zeros(1028)
    args = (1e-3, 0.9, 0.999, 1e-8, 0.1, 1)
    ref = R.adam_reference(w, grad, m, v, *args, split=512)
    bad = R.adam_reference(w, grad, m, v, *args, split=516).master      # the first vector of four past the split decays too
    assert R.old_metric(bad, ref.master) < OLD_TOL
    assert R.worst(bad, ref.master, R.adam_bounds(ref)["master"])[0] > 1.0
