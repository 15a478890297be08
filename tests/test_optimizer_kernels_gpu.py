"""The optimizer kernels of csrc/optimizer.hip through the C ABI: the deterministic sum of squares every replica's clip factor rests on,
both Adam kernels against the float64 AdamW reference of tests/elementwise_ref.py (one step at a time from the kernel's own fp32 state,
under per-element bounds), and the cast kernels of the gradient exchange bit for bit.

Worst err / bound, measured on an MI355X (nothing in these kernels changed with this file, so one column):

    emdr2_sumsq_f32         randn 0.02   1e-12 .. 1e6 0.01   zeros 0.00      n = 1 .. 5,000,003; five runs bit-identical, counter word 0,
                                                                             one scratch shared by alternating grid sizes, out accumulates
    emdr2_adam_step(_flat)  m 0.04  v 0.07  master 0.59 (norm >> clip), 0.25 otherwise      bound of the master: 2.4 ulp (tests/elementwise_ref.py)
                            zero gradient on zero state: master 0.21, not a bit moves where no decay applies
    emdr2_accum_bf16_to_f32 0.50 of one fp32 ulp
    casts                   bit-equal to torch (ties to even, +-0, denormals, +-inf, NaN, FLT_MAX -> inf); widen exact

The work copy is bit-equal to torch's bf16 rounding of the master in every case, and no canary word next to any buffer moved.  The
argument checks of the vector kernels (n % 4, alignment) are in tests/test_abi.py: they need no device.
"""
import pytest
import torch

from tests import elementwise_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CANARY_F32 = 12345.678
CANARY_BF16 = 0x7B7B


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _nat():
    from emdr2_amd import _native
    return _native, _native.lib()


def _assert(tag, ratios):
    print("[opt] %s " % tag + " ".join("%s=%.3f" % (n, r[0]) for n, r in ratios.items()))
    bad = {n: r for n, r in ratios.items() if not r[0] <= 1.0}
    assert not bad, (tag, bad)


# ---- sum of squares -------------------------------------------------------------------------------------------------------------------
def _sumsq_data(fam, n, gen):
    if fam == "randn":
        return torch.randn(n, generator=gen, device=DEV)
    if fam == "wide":                                                    # magnitudes from 1e-12 to 1e6
        return torch.randn(n, generator=gen, device=DEV).sign() * 10.0 ** (-12.0 + 18.0 * torch.rand(n, generator=gen, device=DEV))
    return torch.zeros(n, device=DEV)


def _sumsq(g, out, scratch):
    nat, lib = _nat()
    nat.check(lib.emdr2_sumsq_f32(g.data_ptr(), g.numel(), out.data_ptr(), scratch.data_ptr(), nat.stream_ptr()), "sumsq")


SUMSQ_N = (1, 255, 2049, 2097153, 5000003)                               # 2,097,153: the first n whose blocks take a second lap


@pytest.mark.parametrize("fam", ["randn", "wide", "zero"])
@pytest.mark.parametrize("n", SUMSQ_N)
def test_sumsq_value_determinism_and_counter(n, fam):
    g = _sumsq_data(fam, n, _gen(n))
    scratch = torch.zeros(1025, device=DEV)
    outs = []
    for _ in range(5):
        out = torch.zeros(1, device=DEV)
        _sumsq(g, out, scratch)
        torch.cuda.synchronize()
        outs.append(out)
        assert int(scratch.view(torch.int32)[1024]) == 0                  # the counter word is handed back at 0
    assert all(torch.equal(outs[0].view(torch.int32), o.view(torch.int32)) for o in outs[1:])
    s, bound = R.sumsq_bound(g)
    _assert("sumsq %s n=%d" % (fam, n), {"sumsq": R.worst(outs[0][0], s, bound)})


def test_sumsq_accumulates_and_shares_one_scratch_between_grid_sizes():
    gs = {n: _sumsq_data("randn", n, _gen(n + 1)) for n in SUMSQ_N}
    alone = {}
    for n, g in gs.items():
        out = torch.zeros(1, device=DEV)
        _sumsq(g, out, torch.zeros(1025, device=DEV))
        alone[n] = out
    scratch = torch.zeros(1025, device=DEV)
    order = (5000003, 255, 2097153, 1, 2049, 5000003, 1, 2097153)
    total = torch.zeros(1, device=DEV)
    want = torch.zeros(1, device=DEV)
    for n in order:                                                      # partials of a larger grid are still in the scratch of the next launch
        out = torch.zeros(1, device=DEV)
        _sumsq(gs[n], out, scratch)
        assert torch.equal(out.view(torch.int32), alone[n].view(torch.int32)), n
        _sumsq(gs[n], total, scratch)                                    # out accumulates: += in launch order
        want = want + alone[n]
    torch.cuda.synchronize()
    assert torch.equal(total.view(torch.int32), want.view(torch.int32))
    assert int(scratch.view(torch.int32)[1024]) == 0


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------
def _guarded(n, dtype, fill=None):
    """A length-n view with four canary words on each side (16 bytes for fp32, 8 for bf16: the view keeps the alignment the kernels ask for)."""
    if dtype == torch.float32:
        buf = torch.full((n + 8,), CANARY_F32, device=DEV)
    else:
        buf = torch.full((n + 8,), CANARY_BF16, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    view = buf[4:4 + n]
    if fill is not None:
        view.copy_(fill)
    return buf, view


def _canaries_intact(buf, n):
    if buf.dtype == torch.float32:
        pads = torch.cat([buf[:4], buf[4 + n:]])
        return bool((pads == torch.full_like(pads, CANARY_F32)).all())
    pads = torch.cat([buf[:4], buf[4 + n:]]).view(torch.int16)
    return bool((pads == CANARY_BF16).all())


HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
CLIP_STATES = ("clip0", "null", "below", "above")


def _adam_case(flat, n, split, clip_state, wd):
    nat, lib = _nat()
    g = _gen(n + 13)
    bufs = {}
    views = {}
    for name, init in (("master", torch.randn(n, generator=g, device=DEV)), ("grad", None), ("m", torch.zeros(n, device=DEV)),
                       ("v", torch.zeros(n, device=DEV))):
        bufs[name], views[name] = _guarded(n, torch.float32, init)
    bufs["work"], views["work"] = _guarded(n, torch.bfloat16)
    gsq_buf, gsq = _guarded(1, torch.float32)
    worst = {}
    for step in (1, 2, 100000):
        grad = torch.randn(n, generator=g, device=DEV) * (0.5 if step == 2 else 2.0)
        views["grad"].copy_(grad)
        norm_sq = (grad.double() ** 2).sum().float()
        gsq.copy_(norm_sq.reshape(1))
        norm = float(norm_sq) ** 0.5
        clip = {"clip0": 0.0, "null": 1.0, "below": 10.0 * norm, "above": 0.01 * norm}[clip_state]
        gptr = None if clip_state == "null" else gsq.data_ptr()
        before = {k: views[k].clone() for k in ("master", "m", "v")}
        if flat:
            rc = lib.emdr2_adam_step_flat(views["master"].data_ptr(), views["grad"].data_ptr(), views["m"].data_ptr(), views["v"].data_ptr(),
                                          views["work"].data_ptr(), n, split, HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], wd, step, gptr, clip,
                                          nat.stream_ptr())
        else:
            rc = lib.emdr2_adam_step(views["master"].data_ptr(), views["grad"].data_ptr(), views["m"].data_ptr(), views["v"].data_ptr(),
                                     views["work"].data_ptr(), n, HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], wd, step, gptr, clip, nat.stream_ptr())
        nat.check(rc, "adam")
        torch.cuda.synchronize()
        ref = R.adam_reference(before["master"], grad, before["m"], before["v"], HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], wd, step,
                               None if clip_state == "null" else float(gsq), clip, split if flat else None)
        assert (ref.scale < 1.0) == (clip_state == "above")               # only a norm above the clip scales
        for name, r in R.worst_all({k: views[k] for k in ("master", "m", "v")}, ref, R.adam_bounds(ref)).items():
            if name not in worst or r[0] > worst[name][0]:
                worst[name] = r
        # the bf16 work copy: round-to-nearest-even of the master the kernel wrote
        assert torch.equal(views["work"].view(torch.int16), views["master"].bfloat16().view(torch.int16))
        assert torch.equal(views["grad"], grad)
        for name, buf in bufs.items():
            assert _canaries_intact(buf, n), name
        assert _canaries_intact(gsq_buf, 1)
    _assert("adam%s n=%d split=%s %s wd=%g" % ("_flat" if flat else "", n, split, clip_state, wd), worst)


FLAT_CASES = [(n, split) for n in (4, 1028, 262148) for split in sorted({0, 4, n - 4, n})]


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("clip_state", CLIP_STATES)
@pytest.mark.parametrize("n,split", FLAT_CASES)
def test_adam_step_flat(n, split, clip_state, wd):
    _adam_case(True, n, split, clip_state, wd)


@pytest.mark.parametrize("wd", [0.0, 0.1])
@pytest.mark.parametrize("clip_state", CLIP_STATES)
@pytest.mark.parametrize("n", [4, 1028, 262148])
def test_adam_step(n, clip_state, wd):
    _adam_case(False, n, None, clip_state, wd)


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_adam_zero_gradient_on_zero_state_moves_only_by_the_decay(flat, wd):
    nat, lib = _nat()
    n, split = 1028, 512
    w0 = torch.randn(n, generator=_gen(5), device=DEV)
    master, grad, m, v = w0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    gsq = torch.zeros(1, device=DEV)
    args = (HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], wd, 1, gsq.data_ptr(), 1.0, nat.stream_ptr())
    if flat:
        nat.check(lib.emdr2_adam_step_flat(master.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), None, n, split, *args), "adam_flat")
    else:
        nat.check(lib.emdr2_adam_step(master.data_ptr(), grad.data_ptr(), m.data_ptr(), v.data_ptr(), None, n, *args), "adam")
    torch.cuda.synchronize()
    assert float(m.abs().max()) == 0.0 and float(v.abs().max()) == 0.0
    ref = R.adam_reference(w0, grad, torch.zeros_like(w0), torch.zeros_like(w0), HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], wd, 1, 0.0, 1.0,
                           split if flat else None)
    _assert("adam zero grad flat=%d wd=%g" % (flat, wd), {"master": R.worst(master, ref.master, R.adam_bounds(ref)["master"])})
    still = slice(split, n) if flat else (slice(0, n) if wd == 0.0 else slice(0, 0))
    assert torch.equal(master[still], w0[still])                         # no decay: not a bit moves
    if wd > 0.0:
        assert bool((master[:split] != w0[:split]).any())


# ---- casts ----------------------------------------------------------------------------------------------------------------------------
def _cast_values(n, gen):
    """fp32 values with the cases a float -> bf16 rounding can get wrong in front: ties (to even: down, then up), +-0, fp32 and bf16
    denormals, +-inf, NaN, the largest finite float (rounds to inf), the largest that does not."""
    special = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3.0 * 2.0 ** -8, -(1.0 + 2.0 ** -8), -(1.0 + 3.0 * 2.0 ** -8), 0.0, -0.0, 1.0e-40, -1.0e-40,
                            2.0 ** -130, 2.0 ** -133 * 1.5, float("inf"), float("-inf"), float("nan"), 3.4028234663852886e38,
                            -3.4028234663852886e38, 3.3895313892515355e38 * (1.0 + 2.0 ** -9), 1.0 + 2.0 ** -8 + 2.0 ** -23,
                            1.0 + 2.0 ** -8 - 2.0 ** -24], device=DEV)
    x = torch.randn(n, generator=gen, device=DEV) * 10.0 ** (6.0 * torch.rand(n, generator=gen, device=DEV) - 3.0)
    k = min(n, special.numel())
    x[:k] = special[:k] if n >= special.numel() else special[torch.randperm(special.numel(), generator=gen, device=DEV)[:k]]
    return x


def _same_bf16(got, want):
    """Bit-equal, a NaN matching any NaN."""
    gn, wn = torch.isnan(got), torch.isnan(want)
    return bool((gn == wn).all()) and torch.equal(got.view(torch.int16)[~gn], want.view(torch.int16)[~wn])


@pytest.mark.parametrize("n", [1, 255, 257])
def test_cast_f32_to_bf16_is_round_to_nearest_even(n):
    nat, lib = _nat()
    for seed in range(3 if n == 1 else 1):
        x = _cast_values(n, _gen(n + seed))
        buf, out = _guarded(n, torch.bfloat16)
        nat.check(lib.emdr2_cast_f32_to_bf16(x.data_ptr(), out.data_ptr(), n, nat.stream_ptr()), "cast")
        torch.cuda.synchronize()
        assert _same_bf16(out, x.bfloat16()) and _canaries_intact(buf, n)
    full = _cast_values(257, _gen(9))                                    # every special value, whatever n
    out = torch.empty(257, dtype=torch.bfloat16, device=DEV)
    nat.check(lib.emdr2_cast_f32_to_bf16(full.data_ptr(), out.data_ptr(), 257, nat.stream_ptr()), "cast")
    torch.cuda.synchronize()
    assert _same_bf16(out, full.bfloat16())
    assert bool(torch.isnan(out[12])) and bool(torch.isinf(out[13])) and float(out[0]) == 1.0 and float(out[1]) == 1.0 + 2.0 ** -6


@pytest.mark.parametrize("scale", [1.0, 0.125, 1.0 / 3.0])
@pytest.mark.parametrize("n", [4, 1028])
def test_scale_cast_f32_to_bf16_rounds_the_fp32_product(n, scale):
    nat, lib = _nat()
    x = _cast_values(n, _gen(n))
    buf, out = _guarded(n, torch.bfloat16)
    nat.check(lib.emdr2_scale_cast_f32_to_bf16(x.data_ptr(), out.data_ptr(), n, scale, nat.stream_ptr()), "scale_cast")
    torch.cuda.synchronize()
    want = (x * torch.tensor(scale, dtype=torch.float32, device=DEV)).bfloat16()
    assert _same_bf16(out, want) and _canaries_intact(buf, n)


@pytest.mark.parametrize("n", [4, 1028])
def test_widen_bf16_to_f32_is_exact(n):
    nat, lib = _nat()
    src = _cast_values(n, _gen(n + 2)).bfloat16()
    buf, out = _guarded(n, torch.float32)
    nat.check(lib.emdr2_widen_bf16_to_f32(src.data_ptr(), out.data_ptr(), n, nat.stream_ptr()), "widen")
    torch.cuda.synchronize()
    want = src.float()
    nan = torch.isnan(want)
    assert bool((torch.isnan(out) == nan).all()) and torch.equal(out.view(torch.int32)[~nan], want.view(torch.int32)[~nan])
    assert _canaries_intact(buf, n)


@pytest.mark.parametrize("scale", [1.0, 1.0 / 3.0])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_accum_bf16_to_f32_within_one_ulp(n, scale):
    nat, lib = _nat()
    g = _gen(n + 4)
    src = torch.randn(n, generator=g, device=DEV).bfloat16()
    dst0 = torch.randn(n, generator=g, device=DEV)
    buf, dst = _guarded(n, torch.float32, dst0)
    nat.check(lib.emdr2_accum_bf16_to_f32(src.data_ptr(), dst.data_ptr(), n, scale, nat.stream_ptr()), "accum")
    torch.cuda.synchronize()
    want = dst0.double() + R.f32(scale) * src.double()
    # one fp32 ulp of the largest of result, addend and product (the product may be rounded before the add, or fused into it)
    bound = R._ulp(torch.maximum(torch.maximum(want.abs(), dst0.double().abs()), (R.f32(scale) * src.double()).abs()), 23)
    _assert("accum n=%d scale=%g" % (n, scale), {"dst": R.worst(dst, want, bound)})
    assert _canaries_intact(buf, n)
