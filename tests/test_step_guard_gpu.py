"""GPU: the three kernels of the step guard through the C ABI (include/emdr2_ops.h, "Step guard"; csrc/optimizer.hip), bit for bit: the norm
pass with its census against emdr2_sumsq_f32 and the numpy restatement (tests/step_guard_ref.py), the verdict's state transitions
against the restatement, and the guarded flat Adam against emdr2_adam_step_flat (applied) and against its own inputs (skipped)."""
import numpy as np
import pytest
import torch

from tests import step_guard_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
# 4: one thread's worth; 2048: exactly one block's elements; 2052: a second block with four; the last: 1025 blocks' worth, so the grid is
# capped at 1024 and the stride loop takes a second lap
CENSUS_N = (4, 2048, 2052, 1024 * 2048 + 2048)
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.1)


def _nat():
    from emdr2_amd import _native
    return _native, _native.lib()


def _bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32).cpu()


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


_DATA = {}


def _data(n):
    """Finite gradients of size n, made once per size and never written to."""
    if n not in _DATA:
        _DATA[n] = torch.randn(n, generator=torch.Generator(device=DEV).manual_seed(n), device=DEV)
    return _DATA[n]


def _plain(g, start):
    nat, lib = _nat()
    out, scratch = torch.full((1,), start, device=DEV), torch.zeros(1025, device=DEV)
    nat.check(lib.emdr2_sumsq_f32(g.data_ptr(), g.numel(), out.data_ptr(), scratch.data_ptr(), nat.stream_ptr()), "sumsq")
    return out


def _census(g, start=0.0, bucket=0, census=None):
    nat, lib = _nat()
    out, scratch = torch.full((1,), start, device=DEV), torch.zeros(1025, device=DEV)
    if census is None:
        census = torch.tensor([0, 0, -1, 0], dtype=torch.int64, device=DEV)
    nat.check(lib.emdr2_sumsq_census_f32(g.data_ptr(), g.numel(), out.data_ptr(), scratch.data_ptr(), census.data_ptr(), bucket, nat.stream_ptr()),
              "sumsq_census")
    assert int(scratch[1024:].view(torch.int32)) == 0                    # the counter word is left at zero, like the plain form
    return out, census


@pytest.mark.parametrize("n", CENSUS_N)
def test_census_pass_gives_the_plain_sum_bits_and_an_empty_census_on_finite_data(n):
    g = _data(n)
    for start in (0.0, 3.25):                                            # *out accumulates: a prior bucket's sum
        out, census = _census(g, start)
        assert _same_bits(out, _plain(g, start)), (n, start)
        assert G.words(census) == G.CENSUS_EMPTY


@pytest.mark.parametrize("n", CENSUS_N)
def test_census_counts_and_first_key_equal_the_restatement(n):
    nan, inf = float("nan"), float("inf")
    spots = sorted(set(i for i in (0, n - 1, 2047, 2048) if i < n))      # the ends and the seam between the first two blocks
    plants = [{i: v} for i in spots for v in (nan, inf, -inf)]
    plants += [{spots[0]: inf, spots[-1]: nan}, {spots[-1]: -inf, spots[len(spots) // 2]: nan}]      # two at once
    base = _data(n)
    for bucket, plant in zip([0, 3, 1 << 20] * len(plants), plants):
        g = base.clone()
        for i, v in plant.items():
            g[i] = v
        out, census = _census(g, bucket=bucket)
        assert G.words(census) == G.census(g.cpu().numpy(), bucket), (n, plant)
        ref = _plain(g, 0.0)
        assert not bool(torch.isfinite(out)) and bool(torch.isnan(out)) == bool(torch.isnan(ref))
    # a second bucket's pass merges into the same census
    g = base.clone(); g[n - 1] = nan
    h = base.clone(); h[0] = inf
    _, census = _census(g, bucket=2)
    _, census = _census(h, bucket=1, census=census)
    assert G.words(census) == G.census(h.cpu().numpy(), 1, prior=G.census(g.cpu().numpy(), 2)) == [1, 1, 1 << 40, 0]


def _verdict(gsq, census, state, step):
    nat, lib = _nat()
    nat.check(lib.emdr2_step_verdict(gsq.data_ptr(), census.data_ptr(), state.data_ptr(), step, nat.stream_ptr()), "step_verdict")


def test_squares_that_overflow_are_skipped_with_no_offender():
    g = torch.zeros(2048, device=DEV)
    g[5] = 3e19; g[1999] = 3e19                                          # finite elements; their squares (9e38) are beyond fp32
    out, census = _census(g)
    assert G.words(census) == [0, 0, G.NO_KEY, 0]
    assert bool(torch.isinf(out)) and _same_bits(out, _plain(g, 0.0))
    state = torch.zeros(8, dtype=torch.int64, device=DEV)
    _verdict(out, census, state, 9)
    assert G.words(state) == [1, 1, 1, 1, 9, G.NO_KEY, 0, 0]
    assert G.words(census) == G.CENSUS_EMPTY


def test_verdict_sequence_runs_and_the_sticky_record():
    inf = float("inf")
    seq = [(1.0, G.CENSUS_EMPTY), (float("nan"), [1, 0, 5, 0]), (inf, [0, 2, (1 << 40) | 9, 0]), (2.0, G.CENSUS_EMPTY), (-inf, [3, 1, 7, 0])]
    state, ref = torch.zeros(8, dtype=torch.int64, device=DEV), [0] * 8
    to_i64 = lambda ws: torch.tensor([w - (1 << 64) if w >= (1 << 63) else w for w in ws], dtype=torch.int64, device=DEV)
    for step, (gsq, c) in enumerate(seq, start=1):                       # applied, skip, skip, applied, skip
        census = to_i64(c)
        _verdict(torch.tensor([gsq], device=DEV), census, state, step)
        ref, left = G.verdict(gsq, c, ref, step)
        assert G.words(state) == ref, step
        assert G.words(census) == left == G.CENSUS_EMPTY                 # reset for the next step, whatever the verdict
    assert ref[:4] == [1, 3, 1, 2]                                       # total 3, run 1, longest 2
    assert ref[4:] == [2, 5, 1, 0]                                       # the record of the FIRST skip, not of the later ones
    state[4:8].zero_()                                                   # cleared (FlatAdam.guard_report): the next skip refills it
    _verdict(torch.tensor([4.0], device=DEV), to_i64(G.CENSUS_EMPTY), state, 6)
    assert G.words(state) == [0, 3, 0, 2, 0, 0, 0, 0]
    _verdict(torch.tensor([inf], device=DEV), to_i64([0, 4, 11, 0]), state, 7)
    assert G.words(state) == [1, 4, 1, 2, 7, 11, 0, 4]


def _adam_buffers(n, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda: torch.randn(n, generator=gen, device=DEV)
    buf = {"master": r(), "grad": r(), "m": 0.1 * r(), "v": 0.01 * r().square(), "work": torch.zeros(n, dtype=torch.bfloat16, device=DEV)}
    buf["work"].copy_(buf["master"])
    return buf


def _adam(buf, n, split, gsq, state, step=3, clip=1.0):
    nat, lib = _nat()
    head = (buf["master"].data_ptr(), buf["grad"].data_ptr(), buf["m"].data_ptr(), buf["v"].data_ptr(), buf["work"].data_ptr(), n, split, HYPER["lr"],
            HYPER["b1"], HYPER["b2"], HYPER["eps"], HYPER["wd"], step, gsq.data_ptr(), clip)
    if state is None:
        nat.check(lib.emdr2_adam_step_flat(*head, nat.stream_ptr()), "adam_step_flat")
    else:
        nat.check(lib.emdr2_adam_step_flat_guarded(*head, state.data_ptr(), nat.stream_ptr()), "adam_step_flat_guarded")


@pytest.mark.parametrize("n", (8, 1024, 1028))                           # one thread; one block exactly; a second block with one thread
@pytest.mark.parametrize("where", ("none", "middle", "all"))
def test_guarded_adam_applied_equals_the_plain_entry_and_skipped_stores_nothing(n, where):
    split = {"none": 0, "middle": n // 2 // 4 * 4, "all": n}[where]
    state = torch.zeros(8, dtype=torch.int64, device=DEV)
    # verdict 0: the plain entry's bits, on copies of the same buffers, with a norm above the clip so that the scale enters
    a, b = _adam_buffers(n, 7 * n + split), _adam_buffers(n, 7 * n + split)
    gsq = a["grad"].square().sum().reshape(1)
    assert float(gsq) > 1.0
    _adam(a, n, split, gsq, None)
    _adam(b, n, split, gsq, state)
    for k in ("master", "m", "v", "work"):
        assert _same_bits(a[k], b[k]), k
    assert not _same_bits(a["master"], _adam_buffers(n, 7 * n + split)["master"])          # (it did move)
    # verdict 1 with NaN among the gradients and in the norm: nothing is stored
    c = _adam_buffers(n, 11 * n + split)
    c["grad"][n - 1] = float("nan"); c["grad"][0] = float("inf")
    before = {k: v.clone() for k, v in c.items()}
    state[0] = 1
    _adam(c, n, split, torch.tensor([float("nan")], device=DEV), state)
    torch.cuda.synchronize()
    for k in ("master", "m", "v", "work"):
        assert _same_bits(c[k], before[k]), k
    assert bool(torch.isfinite(c["master"]).all())
