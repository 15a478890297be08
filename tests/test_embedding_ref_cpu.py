"""tests/embedding_ref.py checked without a GPU: the host restatement of csrc/rng.h, the fp32 torch implementation of the op against
every bound on every family (worst ratios printed; the table in the module docstring of embedding_ref.py is what this file measured),
and planted faults that the old whole-tensor metric max|a - r| / max|r| < 2e-2 passes and the per-element bounds catch -- each asserted
both ways."""
import math

import numpy as np
import pytest
import torch

from tests import embedding_ref as E

PS = (0.0, 1e-6, 0.1, 0.5)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _case(idfam, dfam, tfam, nseq, S, H, p, seed):
    g = _gen(seed)
    n = nseq * S
    V = E.vocab_for(idfam, n)
    ids = E.ids_inputs(idfam, n, V, g)
    types, nt = E.types_inputs(tfam, n, g)
    W, P, T = E.tables(V, S + 2, nt, H, g)
    dout = E.dout_inputs(dfam, ids, H, g)
    keep = E.keep_bits(n, H, p, seed) if p > 0 else None
    r = E.embedding_reference(ids.reshape(nseq, S), types, W, P, T, keep, E.keep_scale_exact(p) if p > 0 else 1.0, dout)
    return r, W, P, T, dout


# ---- the rng restatement ------------------------------------------------------------------------------------------------------------------
def test_threshold_and_scale():
    assert E.drop_thr(1e-6) == 0 and E.keep_scale_f32(1e-6) == 1.0 and E.keep_scale_exact(1e-6) == 1.0
    assert bool(E.keep_bits(64, 264, 1e-6, 5).all())
    assert E.drop_thr(0.1) == 6554 and E.drop_thr(0.5) == 32768
    assert E.keep_scale_exact(0.1) == 65536.0 / 58982.0 and E.keep_scale_exact(0.5) == 2.0
    assert abs(E.keep_scale_f32(0.1) - E.keep_scale_exact(0.1)) <= 2.0 ** -24 * E.keep_scale_exact(0.1)
    assert abs(E.keep_scale_exact(0.1) - 1.0 / 0.9) > 100 * 2.0 ** -24      # why the float64 reference uses the rational


@pytest.mark.parametrize("seed", [0, 2 ** 32 - 1, 0x51])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_keep_rate(p, seed):
    rows, cols = 4096, 768
    k = E.keep_bits(rows, cols, p, seed)
    q = E.drop_thr(p) / 65536.0
    rate, sigma = 1.0 - float(k.double().mean()), math.sqrt(q * (1.0 - q) / (rows * cols))
    print("[emb-ref] p=%g seed=%d drop rate %.6f (quantised p %.6f, %.2f sigma)" % (p, seed, rate, q, abs(rate - q) / sigma))
    assert abs(rate - q) <= 5.0 * sigma
    for sub in (k[:, 0::2], k[:, 1::2], k[0::2], k[1::2]):                  # neither half of a pair nor a row parity is biased
        assert abs(1.0 - float(sub.double().mean()) - q) <= 5.0 * sigma * math.sqrt(2.0)


def test_pair_halves_and_row_hash():
    rh = E.row_hash(7, np.arange(5, dtype=np.uint64))
    cols = np.arange(16, dtype=np.uint32)
    b = E.pair_bits(rh[:, None], cols[None, :])
    assert np.array_equal(b[:, 0::2], b[:, 1::2])                           # the two columns of a pair share their 32 bits
    for thr in (1, 6554, 32768, 65535):
        k = E.keep(rh[:, None], cols[None, :], thr)
        assert np.array_equal(k[:, 0::2], (b[:, 0::2] & np.uint32(0xffff)) >= thr)      # even column: the low half
        assert np.array_equal(k[:, 1::2], (b[:, 1::2] >> np.uint32(16)) >= thr)         # odd column: the high half
    # one value by hand, in Python integers: mix32 and the row hash of (seed 1, row 2)
    def mix(x):
        x ^= x >> 16; x = x * 0x7feb352d & 0xffffffff; x ^= x >> 15; x = x * 0x846ca68b & 0xffffffff; x ^= x >> 16
        return x
    assert int(E.mix32(123456789)[0]) == mix(123456789)
    assert int(E.row_hash(1, [2])[0]) == mix(2 ^ mix((0 + 1 * 0x9e3779b9 + 0x85ebca6b) & 0xffffffff))
    assert int(E.row_hash(1, [2 ** 32 + 2])[0]) == mix(2 ^ mix((1 + 1 * 0x9e3779b9 + 0x85ebca6b) & 0xffffffff))   # the high word counts
    assert not np.array_equal(E.row_hash(0, np.arange(64)), E.row_hash(2 ** 32 - 1, np.arange(64)))


# ---- the fp32 torch implementation stays within every bound -----------------------------------------------------------------------------
WORST = {}


def _note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)


@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("idfam", E.IDS_FAMILIES)
def test_torch_f32_within_bounds(idfam, p):
    """Every dout and types family, bf16 out with dropout p and (at p = 0) the fp32 twin; the exact family at p = 0."""
    for dfam in E.DOUT_FAMILIES + (E.EXACT_DOUT_FAMILIES if p == 0.0 else ()):
        for tfam in E.TYPES_FAMILIES:
            for (nseq, S, H) in ((37, 8, 8), (300, 4, 264)) if tfam in ("none", "t4", "skip_of_4") else ((37, 8, 8),):
                r, W, P, T, dout = _case(idfam, dfam, tfam, nseq, S, H, p, 11)
                sc = E.keep_scale_f32(p) if p > 0 else 1.0
                for fp32 in ((False, True) if p == 0.0 else (False,)):
                    got = E.embedding_torch_f32(r, W, P, T, dout, sc, store_bf16=not fp32)
                    B = E.embedding_bounds(r, *((E.C_F32, 23) if fp32 else (E.C_BF16, 7)))
                    for n in B:
                        ratio, idx = E.worst(got[n], getattr(r, n), B[n])
                        _note(("out_f32" if fp32 else "out_bf16") if n == "out" else n, ratio)
                        assert ratio <= 0.5, (idfam, dfam, tfam, nseq, S, H, p, fp32, n, ratio, idx)
                    assert bool((got["out"][~r.kept] == 0).all())
                    if dfam == "coded":
                        for n in B:
                            if n != "out":
                                assert torch.equal(got[n].double(), getattr(r, n)), (idfam, tfam, n)
                    if tfam == "skip_of_4":
                        assert float(r.aT[2].max()) == 0.0 and float(E.embedding_bounds(r)["dT"][2].max()) == 0.0
    print("[emb-ref] worst ratios of the fp32 torch reference so far: " + " ".join("%s=%.3f" % kv for kv in sorted(WORST.items())))


# ---- planted faults -----------------------------------------------------------------------------------------------------------------------
def _planted(nseq=300, S=4, H=264, p=0.1, seed=3):
    """zipf ids, four types, and the padding-like structure of the issue: the tokens at position 0 all carry the heavy id and type 0 and a
    gradient 2^10 in magnitude; every other token's gradient is 2^-6 .. 2^-20 by id, the once-seen ids 2^-20, type 3 only on a few quiet
    tokens.  One heavy row per table then owns max|r| of dW, dP and dT."""
    g = _gen(seed)
    n = nseq * S
    V = 64
    ids = E.ids_inputs("zipf", n, V, g).reshape(nseq, S)
    ids[:, 0] = E.HEAVY_ID                                                  # (a once-seen id that sat at position 0 is simply gone)
    types = torch.randint(0, 3, (nseq, S), generator=g)
    types[:, 0] = 0
    types[5::7, S - 1] = 3
    W, P, T = E.tables(V, S + 2, 4, H, g)
    e = -6.0 - ((ids * 7) % 15).double()
    e = torch.where(ids >= V - 5, torch.full_like(e, -20.0), e)
    e[:, 0] = 10.0
    dout = E.bf((torch.randn((nseq, S, H), generator=g) * torch.exp2(e).float()[..., None]).reshape(n, H))
    keep = E.keep_bits(n, H, p, seed) if p > 0 else None
    scale = E.keep_scale_exact(p) if p > 0 else 1.0
    r = E.embedding_reference(ids, types.reshape(-1), W, P, T, keep, scale, dout)
    good = E.embedding_torch_f32(r, W, P, T, dout, E.keep_scale_f32(p) if p > 0 else 1.0)
    return r, good, (ids, types, W, P, T, dout, keep)


def _both_ways(r, good, bad, name, tag):
    B = E.embedding_bounds(r)
    ref = getattr(r, name)
    ok, _ = E.worst(good[name], ref, B[name])
    ratio, idx = E.worst(bad[name], ref, B[name])
    om = E.old_metric(bad[name], ref)
    print("[emb-ref] planted %-34s %s: old metric %.2e (passes < 2e-2), new ratio %.3g at %s (unplanted %.3f)" % (tag, name, om, ratio, idx, ok))
    assert ok <= 0.5
    assert om < 2e-2, (tag, om)
    assert ratio > 1.0, (tag, ratio)


def test_planted_once_seen_row_dropped():
    r, good, (ids, *_rest) = _planted()
    rare = int((torch.bincount(ids.reshape(-1), minlength=64) == 1).nonzero()[-1])
    bad = dict(good); bad["dW"] = good["dW"].clone(); bad["dW"][rare] = 0.0
    assert float(r.aW[rare].max()) > 0
    _both_ways(r, good, bad, "dW", "once-seen token's dW row dropped")


def test_planted_position_row_first_256_sequences_only():
    r, good, (ids, types, W, P, T, dout, keep) = _planted()
    nseq, S = ids.shape
    g = (r.term.float()).reshape(nseq, S, -1)
    bad = dict(good); bad["dP"] = good["dP"].clone(); bad["dP"][S - 1] = g[:256, S - 1].sum(0)
    _both_ways(r, good, bad, "dP", "position row S-1 over 256 sequences")


def test_planted_type_row_3_ignored():
    r, good, _ = _planted()
    bad = dict(good); bad["dT"] = good["dT"].clone(); bad["dT"][3] = 0.0
    assert float(r.aT[3].max()) > 0
    _both_ways(r, good, bad, "dT", "type row 3 ignored")


def test_planted_second_column_block_of_a_position_row_zero():
    r, good, _ = _planted()
    bad = dict(good); bad["dP"] = good["dP"].clone(); bad["dP"][2, 256:] = 0.0
    _both_ways(r, good, bad, "dP", "columns >= 256 of dP row 2 zero")


def test_planted_backward_mask_shifted_by_one_pair():
    """The backward takes the bits of the NEXT column pair.  Position 0 carries a gradient of one sign here (|randn| + 1), so the heavy
    rows are sums of 1,200 like terms and the wrong 10 % of them (p = 0.01: a dozen of them) is a small relative change there, as the old metric sees it."""
    p, nseq, S, H, seed = 0.01, 1200, 2, 16, 3
    r, good, (ids, types, W, P, T, dout, keep) = _planted(nseq, S, H, p, seed)
    d3 = dout.reshape(nseq, S, H).clone()
    d3[:, 0] = E.bf(d3[:, 0].abs() + 1024.0)
    dout = d3.reshape(-1, H)
    r = E.embedding_reference(ids, types.reshape(-1), W, P, T, keep, E.keep_scale_exact(p), dout)
    good = E.embedding_torch_f32(r, W, P, T, dout, E.keep_scale_f32(p))
    shifted = torch.roll(keep, -2, dims=1)
    rs = E.embedding_reference(ids, types.reshape(-1), W, P, T, shifted, E.keep_scale_exact(p), dout)
    bad = E.embedding_torch_f32(rs, W, P, T, dout, E.keep_scale_f32(p))
    for name in ("dW", "dP", "dT"):
        _both_ways(r, good, bad, name, "backward mask shifted by a pair")


def test_planted_keep_scale_one_over_one_minus_p():
    r, good, (ids, types, W, P, T, dout, keep) = _planted(p=0.1)
    bad = E.embedding_torch_f32(r, W, P, T, dout, float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))))
    for name in ("dW", "dP", "dT"):
        B = E.embedding_bounds(r)[name]
        ratio, _ = E.worst(bad[name], getattr(r, name), B)
        print("[emb-ref] planted keep scale 1 / (1 - p) %s: old metric %.2e, new ratio %.3g" % (name, E.old_metric(bad[name], getattr(r, name)), ratio))
        assert E.old_metric(bad[name], getattr(r, name)) < 2e-2
    _both_ways(r, good, bad, "dW", "keep scale 1 / (1 - p)")               # 6.4e-6 = 107 u: seen on every row of fewer than ~100 terms


def test_planted_minus_zero_row_lands_in_an_untouched_row():
    """IEEE addition of -0.0 ONTO a value changes no bit of it (x + -0.0 == x, and +0.0 + -0.0 == +0.0), so the fault that a skipped
    `-0.0` row can cause is a STORE of its sum: the untouched row of a zero-initialised table becomes -0.0.  Numerically nothing
    changed (the worst ratio is 0 and the old metric is 0); the bits did."""
    g = _gen(9)
    n, H, V = 64, 8, 16
    ids = torch.randint(1, V - 1, (n,), generator=g)
    ids[5] = V - 1                                                          # the only token of the last row ...
    W, P, T = E.tables(V, 10, 0, H, g)
    dout = E.bf(torch.randn((n, H), generator=g))
    dout[5] = -0.0                                                          # ... and its gradient is a row of -0.0
    r = E.embedding_reference(ids.reshape(8, 8), None, W, P, None, None, 1.0, dout)
    before = {"dW": torch.zeros_like(W), "dP": torch.zeros_like(P)}
    good = E.embedding_torch_f32(r, W, P, None, dout, 1.0)
    assert float(r.aW[V - 1].max()) == 0.0
    res = E.worst_grads(good, before, r, E.embedding_bounds(r))
    assert res["dW"][0] <= 0.5 and res["dP"][0] <= 0.5
    bad = dict(good); bad["dW"] = good["dW"].clone(); bad["dW"][V - 1] = dout[5]
    assert torch.equal(bad["dW"], good["dW"]) and E.old_metric(bad["dW"], r.dW) == 0.0 and E.worst(bad["dW"], r.dW, E.embedding_bounds(r)["dW"])[0] == 0.0
    assert not E.untouched_ok(bad["dW"], before["dW"], r.aW)
    assert E.worst_grads(bad, before, r, E.embedding_bounds(r))["dW"][0] == float("inf")
    # a sentinel pre-fill with -0.0 elements: an accumulation that adds only its non-zero terms leaves every other element's bits, and
    # worst_grads accepts it; one that adds the +0.0 of a token-less element turns the -0.0 into +0.0 and is caught, on bits alone
    sent = {"dW": E.sentinel(W.shape), "dP": E.sentinel(P.shape)}
    acc = {k: torch.where(good[k] != 0, sent[k] + good[k], sent[k]) for k in sent}
    assert E.worst_grads(acc, sent, r, E.embedding_bounds(r))["dW"][0] <= 1.0
    adds_zeros = {k: sent[k] + good[k] for k in sent}
    assert torch.equal(adds_zeros["dW"], acc["dW"]) and E.worst_grads(adds_zeros, sent, r, E.embedding_bounds(r))["dW"][0] == float("inf")
    assert bool(E.same_bits(acc["dP"][8:], sent["dP"][8:]).all())          # P rows >= S


def test_packed_reference_matches_dense_at_real_positions():
    """The packed form of the reference (cu, rowmap, zero tail rows) against its dense form."""
    g = _gen(4)
    nseq, S, H, V = 9, 8, 8, 64
    lens = torch.tensor([1, 8, 3, 8, 5, 2, 8, 1, 7])
    ids = E.ids_inputs("uniform", nseq * S, V, g, lo=1).reshape(nseq, S)
    ids = torch.where(torch.arange(S)[None] < lens[:, None], ids, torch.zeros_like(ids))
    real = ids != 0
    cu = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).int()
    total, rows = int(cu[-1]), 48
    rowmap = torch.full((rows,), -1, dtype=torch.int32)
    rowmap[:total] = torch.arange(nseq * S).reshape(nseq, S)[real].int()
    pid = torch.zeros(rows, dtype=torch.int64); pid[:total] = ids[real]
    W, P, T = E.tables(V, S, 0, H, g)
    dd = E.bf(torch.randn((nseq * S, H), generator=g)) * real.reshape(-1, 1)
    dp = torch.zeros((rows, H)); dp[:total] = dd[real.reshape(-1)]
    rd = E.embedding_reference(ids, None, W, P, None, None, 1.0, dd)
    rp = E.embedding_reference(pid, None, W, P, None, None, 1.0, dp, S=S, cu=cu, rowmap=rowmap)
    assert torch.equal(rp.out[:total], rd.out[real.reshape(-1)]) and bool((rp.out[total:] == 0).all())
    assert torch.allclose(rp.dP, rd.dP, rtol=0, atol=1e-12) and torch.allclose(rp.dW[1:], rd.dW[1:], rtol=0, atol=1e-12)
    assert float(rp.aW[0].max()) == 0.0                                     # the tail rows' id 0 adds nothing
