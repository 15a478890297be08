"""The ordered-sum gradient entries through the C ABI (include/emdr2_ops.h, "Ordered sums"): emdr2_gemm_tn_bf16_ordered,
emdr2_layernorm_bwd_ordered, emdr2_embedding_bwd_ordered.  Four properties per entry and case:

  value           within the derived bound of the float64 restatement (tests/ordered_grads_ref.py: gamma_n sum |term|, nothing measured)
  repeatability   three calls on the same inputs give identical bits, on data where the order of a sum shows (magnitudes over 2^+-20)
  one add         into zeros -> t; into a destination pre-filled with p -> exactly fl32(p + t).  With p = 2^24 and contributions of 1.0 a sum
                  that adds its parts onto the destination one by one stays at 2^24: an atomic or slice-by-slice implementation fails here
  untouched       vocabulary rows without tokens and positions no sequence reaches keep a NaN payload and -0.0 bit for bit

Every output and the workspace sit between guard words that must not change.  Shapes: the smallest at which each path can go wrong (tile tails,
3 x 3 tiles, uneven and capped slices, one slice; 1 .. 16,391 LayerNorm rows = more than the 2,048 workgroups' worth; embedding runs of
C - 1, C, C + 1, 2 C + 1 tokens for the chunk constant C = 128)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import embedding_ref as E
from tests import ordered_grads_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
CHUNK = 128                                    # EMB_CHUNK of csrc/embedding.hip
NAN_PAYLOAD = 0x7fc12345
NEG_ZERO = 0x80000000


@pytest.fixture(scope="module")
def lib():
    from emdr2_amd import _native
    return _native.lib()


def _sp():
    from emdr2_amd import _native
    return _native.stream_ptr()


class Guarded(object):
    """A device buffer between two runs of guard words."""

    def __init__(self, n, dtype, fill=None, guard_bits=0x5a):
        self.full = torch.empty(n + 2 * GUARD, dtype=dtype, device=DEV)
        self.full.view(torch.uint8).fill_(guard_bits)
        self.v = self.full[GUARD:GUARD + n]
        self.edges = torch.cat([self.full[:GUARD], self.full[GUARD + n:]]).clone()
        if fill is not None:
            self.v.copy_(fill if torch.is_tensor(fill) else torch.as_tensor(fill, device=DEV).to(dtype).expand(n))

    def intact(self):
        e = torch.cat([self.full[:GUARD], self.full[GUARD + self.v.numel():]])
        return torch.equal(e.view(torch.uint8), self.edges.view(torch.uint8))

    def ptr(self):
        return self.v.data_ptr()


def _dev_bf16(a):
    return torch.from_numpy(R.bf16_bits(a)).to(DEV).view(torch.bfloat16)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def _nbytes(fn, *args):
    n = ctypes.c_size_t()
    assert fn(*(args + (ctypes.byref(n),))) == 0
    return n.value


def _fl32_add(p, t):
    return (p.astype(np.float32) + t.astype(np.float32)).astype(np.float32)


def _within(got, ref, bound, what):
    err, bound = np.abs(got.astype(np.float64) - ref), np.broadcast_to(bound, ref.shape)
    assert not err[bound == 0].any(), what                           # a destination without terms: exact
    ratio = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    print("%s: worst err / bound = %.3f" % (what, ratio))
    assert ratio <= 1.0, (what, ratio)


def _same(a, b, what):
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), what


# ---- weight-gradient GEMM -----------------------------------------------------------------------------------------------------------------------
def _tn(lib, A, B, I, J, R_, split, C, ldc, colsum, ws):
    rc = lib.emdr2_gemm_tn_bf16_ordered(A.data_ptr(), I, B.data_ptr(), J, C.ptr(), ldc, I, J, R_, split, colsum.ptr() if colsum is not None else None,
                                        ws.ptr(), ws.v.numel(), _sp())
    assert rc == 0, rc
    torch.cuda.synchronize()


def _tn_run(lib, A, B, I, J, R_, split, ldc, with_cs, prefill_c=0.0, prefill_cs=0.0):
    C = Guarded(I * ldc, torch.float32, prefill_c)
    cs = Guarded(I, torch.float32, prefill_cs) if with_cs else None
    ws = Guarded(max(_nbytes(lib.emdr2_gemm_tn_ordered_ws_bytes, I, J, R_, split), 16), torch.uint8)
    _tn(lib, A, B, I, J, R_, split, C, ldc, cs, ws)
    assert C.intact() and ws.intact() and (cs is None or cs.intact())
    c = C.v.cpu().numpy().reshape(I, ldc)
    return c, (cs.v.cpu().numpy() if with_cs else None)


# (R, split): 64-row kernel with uneven slices; general kernel with 2 slices and with more slices than chunks; capped to one slice; one slice of each
TN_SPLITS = ((320, 3), (96, 2), (96, 4), (64, 5), (320, 1), (96, 1))
TN_SHAPES = ((8, 8), (264, 520), (520, 264), (520, 520))


@pytest.mark.parametrize("I,J", TN_SHAPES)
@pytest.mark.parametrize("R_,split", TN_SPLITS)
def test_gemm_tn_ordered(lib, R_, split, I, J):
    case = TN_SPLITS.index((R_, split)) + TN_SHAPES.index((I, J))
    with_cs, ldc = case % 2 == 0, J + (8 if case % 3 == 0 else 0)
    rng = np.random.default_rng(100 + case)
    a, b = R.spread((R_, I), rng), R.spread((R_, J), rng)
    A, B = _dev_bf16(a), _dev_bf16(b)
    dW, S, cs, Scs = R.tn_reference(a, b)
    # value + repeatability
    runs = [_tn_run(lib, A, B, I, J, R_, split, ldc, with_cs) for _ in range(3)]
    t, tcs = runs[0]
    _within(t[:, :J], dW, R.sum_bound(S, R_ + split), "dW")
    if ldc > J:
        assert not t[:, J:].any()                                    # the pad columns of C are not the entry's
    if with_cs:
        _within(tcs, cs, R.sum_bound(Scs, R_ + split), "colsum")
    for c2, cs2 in runs[1:]:
        _same(c2, t, "dW repeat")
        if with_cs:
            _same(cs2, tcs, "colsum repeat")
    # one add per destination: a spread pre-fill
    p = R.spread((I, ldc), rng, -10, 30)
    pcs = R.spread((I,), rng, -10, 30)
    got, gotcs = _tn_run(lib, A, B, I, J, R_, split, ldc, with_cs, torch.from_numpy(p.reshape(-1)).to(DEV), torch.from_numpy(pcs).to(DEV))
    _same(got[:, :J], _fl32_add(p[:, :J], t[:, :J]), "dW = fl32(p + t)")
    _same(got[:, J:], p[:, J:], "pad columns")
    if with_cs:
        _same(gotcs, _fl32_add(pcs, tcs), "colsum = fl32(p + t)")
    # ... and 2^24 with one contribution of 1.0 per 32-row chunk
    a1 = np.zeros((R_, I), dtype=np.float32); a1[::32] = 1.0
    b1 = np.zeros((R_, J), dtype=np.float32); b1[::32] = 1.0
    A1, B1 = _dev_bf16(a1), _dev_bf16(b1)
    t1, tcs1 = _tn_run(lib, A1, B1, I, J, R_, split, ldc, with_cs)
    assert np.all(t1[:, :J] == R_ // 32) and (not with_cs or np.all(tcs1 == R_ // 32))
    g1, gcs1 = _tn_run(lib, A1, B1, I, J, R_, split, ldc, with_cs, 2.0 ** 24, 2.0 ** 24)
    want = np.float32(2.0 ** 24) + np.float32(R_ // 32)
    assert np.all(g1[:, :J] == want), (g1[0, 0], want)
    assert not with_cs or np.all(gcs1 == want)


# ---- LayerNorm backward ---------------------------------------------------------------------------------------------------------------------------
def _ln_inputs(rows, H, seed):
    rng = np.random.default_rng(seed)
    x = R.to_bf16(rng.standard_normal((rows, H)) * 2.0 + 0.5)
    dy = R.spread((rows, H), rng)
    mean = x.astype(np.float64).mean(1).astype(np.float32)
    rstd = (1.0 / np.sqrt(x.astype(np.float64).var(1) + 1e-5)).astype(np.float32)
    gamma = (1.0 + 0.1 * rng.standard_normal(H)).astype(np.float32)
    dres = R.to_bf16(rng.standard_normal((rows, H)))
    return x, dy, mean, rstd, gamma, dres


def _ln_call(lib, t, rows, H, use_dres, mask_p, ordered, pre_g=0.0, pre_b=0.0):
    dx = Guarded(rows * H, torch.bfloat16)
    dm = Guarded(rows * H, torch.bfloat16) if mask_p else None
    dg, db = Guarded(H, torch.float32, pre_g), Guarded(H, torch.float32, pre_b)
    common = (t["dy"].data_ptr(), t["x"].data_ptr(), t["gamma"].data_ptr(), t["mean"].data_ptr(), t["rstd"].data_ptr(),
              t["dres"].data_ptr() if use_dres else None, dx.ptr(), dg.ptr(), db.ptr(), rows, H)
    if ordered:
        ws = Guarded(_nbytes(lib.emdr2_layernorm_bwd_ordered_ws_bytes, rows, H), torch.uint8)
        rc = lib.emdr2_layernorm_bwd_ordered(*(common + (dm.ptr() if dm else None, mask_p, 77, ws.ptr(), ws.v.numel(), _sp())))
    elif mask_p:
        ws = None
        rc = lib.emdr2_layernorm_bwd_mask(*(common + (dm.ptr(), mask_p, 77, _sp())))
    else:
        ws = None
        rc = lib.emdr2_layernorm_bwd(*(common + (_sp(),)))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert dx.intact() and dg.intact() and db.intact() and (dm is None or dm.intact()) and (ws is None or ws.intact())
    return (dx.v.view(torch.int16).cpu().numpy(), dm.v.view(torch.int16).cpu().numpy() if dm else None, dg.v.cpu().numpy(), db.v.cpu().numpy())


LN_CASES = [(768, r) for r in (1, 2, 3, 9, 4097, 16391)] + [(264, r) for r in (1, 31, 33, 1000)]


@pytest.mark.parametrize("H,rows", LN_CASES)
@pytest.mark.parametrize("variant", ("plain", "dres_mask"))
def test_layernorm_bwd_ordered(lib, H, rows, variant):
    use_dres = variant == "dres_mask"
    mask_p = 0.1 if (use_dres and H == 768) else 0.0                  # the mask exists on the 768 path only (-4 elsewhere, checked below)
    x, dy, mean, rstd, gamma, dres = _ln_inputs(rows, H, 7 * rows + H)
    t = dict(x=_dev_bf16(x), dy=_dev_bf16(dy), dres=_dev_bf16(dres), mean=torch.from_numpy(mean).to(DEV), rstd=torch.from_numpy(rstd).to(DEV),
             gamma=torch.from_numpy(gamma).to(DEV))
    dg64, Sg, db64, Sb = R.ln_reference(dy, x, mean, rstd)
    runs = [_ln_call(lib, t, rows, H, use_dres, mask_p, True) for _ in range(3)]
    dx, dm, dg, db = runs[0]
    _within(dg, dg64, R.sum_bound(Sg, rows, e_term=R.E_XHAT), "dgamma")
    _within(db, db64, R.sum_bound(Sb, rows), "dbeta")
    for r in runs[1:]:
        _same(r[2], dg, "dgamma repeat"); _same(r[3], db, "dbeta repeat")
    # dx (and dmask) are the bits of the existing entries on the same inputs
    odx, odm, _, _ = _ln_call(lib, t, rows, H, use_dres, mask_p, False)
    assert np.array_equal(dx, odx) and (dm is None or np.array_equal(dm, odm))
    if use_dres and H != 768:
        dxg, dmg = Guarded(rows * H, torch.bfloat16), Guarded(rows * H, torch.bfloat16)
        g = Guarded(H, torch.float32, 0.0)
        assert lib.emdr2_layernorm_bwd_ordered(t["dy"].data_ptr(), t["x"].data_ptr(), t["gamma"].data_ptr(), t["mean"].data_ptr(), t["rstd"].data_ptr(), None,
                                               dxg.ptr(), g.ptr(), g.ptr(), rows, H, dmg.ptr(), 0.1, 77, g.ptr(), 1 << 30, _sp()) == -4
    # one add per destination
    rng = np.random.default_rng(rows)
    pg, pb = R.spread((H,), rng, -10, 30), R.spread((H,), rng, -10, 30)
    _, _, gg, gb = _ln_call(lib, t, rows, H, use_dres, mask_p, True, torch.from_numpy(pg).to(DEV), torch.from_numpy(pb).to(DEV))
    _same(gg, _fl32_add(pg, dg), "dgamma = fl32(p + t)"); _same(gb, _fl32_add(pb, db), "dbeta = fl32(p + t)")
    # 2^24 and dy = 1: dbeta's contributions are 1.0 each
    t1 = dict(t, dy=_dev_bf16(np.ones((rows, H), dtype=np.float32)))
    _, _, _, b0 = _ln_call(lib, t1, rows, H, use_dres, mask_p, True)
    assert np.all(b0 == rows)
    _, _, _, b1 = _ln_call(lib, t1, rows, H, use_dres, mask_p, True, 0.0, 2.0 ** 24)
    assert np.all(b1 == np.float32(2.0 ** 24) + np.float32(rows)), (b1[0], rows)


# ---- embedding backward ---------------------------------------------------------------------------------------------------------------------------
def _ids_pattern(pattern, n, rng):
    """-> ids [n] (in a shuffled token order) over a vocabulary that has rows without tokens"""
    if pattern == "one":
        ids = np.full(n, 5)
    elif pattern == "distinct":
        ids = 3 + 2 * rng.permutation(n)                              # every odd row stays empty
    elif pattern == "two":
        ids = np.where(rng.random(n) < 0.3, 2, 9)
    else:                                                             # runs of C - 1, C, C + 1, 2 C + 1 tokens, the rest distinct
        runs = [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
        ids = np.concatenate([np.full(m, 4 + 3 * k) for k, m in enumerate(runs)] + [100 + 2 * np.arange(max(n - sum(runs), 0))])[:n]
        ids = rng.permutation(ids)
    return ids.astype(np.int64)


def _emb_case(pattern, H, S, packed, n_types, drop_p, seed):
    rng = np.random.default_rng(seed)
    need = 5 * CHUNK + 1 if pattern == "runs" else 3 * S
    if packed:
        lens = list(range(1, S - 1)) + [3]                            # positions S - 2 and S - 1: nobody reaches them
        while sum(lens) < need:
            lens += [max(S - 2, 1)]
        total = sum(lens)
        rows = (total + 31) // 32 * 32 + 32                           # at least 32 tail rows (id 0, zero gradient)
        pos = np.full(rows, -1)
        cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        for b, ln in enumerate(lens):
            pos[cu[b]:cu[b + 1]] = np.arange(ln)
        nseq = len(lens)
    else:
        nseq = (need + S - 1) // S
        rows = total = nseq * S
        pos, cu = np.tile(np.arange(S), nseq), None
    ids = np.zeros(rows, dtype=np.int64)
    ids[:total] = _ids_pattern(pattern, total, rng)
    types = None
    if n_types:
        types = np.zeros(rows, dtype=np.int64)
        types[:total] = rng.integers(0, n_types, total)
    dout = R.spread((rows, H), rng)
    dout[total:] = 0.0
    dout[rng.random(rows) < 0.1] = 0.0                                # some zero rows among the real ones
    return dict(ids=ids, types=types, dout=dout, pos=pos, cu=cu, nseq=nseq, rows=rows, total=total, V=int(ids.max()) + 3, P_rows=S + 2,
                keep=E.keep_bits(rows, H, drop_p, seed).numpy(), scale=E.keep_scale_f32(drop_p) if drop_p > 0 else 1.0)


def _emb_call(lib, c, t, H, S, n_types, drop_p, seed, pre):
    out = {k: Guarded(v.size, torch.float32, torch.from_numpy(v.reshape(-1)).to(DEV)) for k, v in pre.items()}
    ws = Guarded(_nbytes(lib.emdr2_embedding_bwd_ordered_ws_bytes, c["rows"], c["nseq"], S, H, n_types), torch.uint8)
    rc = lib.emdr2_embedding_bwd_ordered(t["ids"].data_ptr(), t["types"].data_ptr() if n_types else None, t["cu"].data_ptr() if c["cu"] is not None else None,
                                         c["nseq"], t["order"].data_ptr(), t["dout"].data_ptr(), out["dW"].ptr(), out["dP"].ptr(),
                                         out["dT"].ptr() if n_types else None, c["rows"], S, H, n_types, drop_p, seed, ws.ptr(), ws.v.numel(), _sp())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert ws.intact() and all(g.intact() for g in out.values())
    return {k: g.v.cpu().numpy().reshape(pre[k].shape) for k, g in out.items()}


EMB_CASES = [(H, S, pattern, packed) for H in (32, 768) for S in (8, 48) for pattern in ("one", "distinct", "two", "runs") for packed in (False, True)]


@pytest.mark.parametrize("H,S,pattern,packed", EMB_CASES)
def test_embedding_bwd_ordered(lib, H, S, pattern, packed):
    k = EMB_CASES.index((H, S, pattern, packed))
    n_types, drop_p, seed = k % 5, (0.1 if k % 2 else 0.0), 1000 + k          # types: none, then 1 .. 4 tables
    c = _emb_case(pattern, H, S, packed, n_types, drop_p, seed)
    ids_t = torch.from_numpy(c["ids"]).to(DEV)
    t = dict(ids=ids_t, order=torch.sort(ids_t, stable=True)[1], dout=_dev_bf16(c["dout"]),
             types=torch.from_numpy(c["types"]).to(DEV) if n_types else None, cu=torch.from_numpy(c["cu"]).to(DEV) if packed else None)
    ref = R.embedding_reference(c["ids"], c["types"], c["dout"], c["keep"], c["scale"], c["pos"], c["V"], c["P_rows"], n_types)
    shapes = {"dW": (c["V"], H), "dP": (c["P_rows"], H)}
    if n_types:
        shapes["dT"] = (n_types, H)
    zeros = {k_: np.zeros(s, dtype=np.float32) for k_, s in shapes.items()}
    runs = [_emb_call(lib, c, t, H, S, n_types, drop_p, seed, zeros) for _ in range(3)]
    e_term = R.gamma(1) if drop_p > 0 else 0.0
    for name in shapes:
        s64, maj, cnt = ref[name]
        _within(runs[0][name], s64, R.sum_bound(maj, cnt[:, None].astype(np.float64), e_term=e_term), name)
        for r in runs[1:]:
            _same(r[name], runs[0][name], name + " repeat")
    # one add per destination, and destinations nobody contributes to: a NaN payload on even columns, -0.0 on odd ones
    rng = np.random.default_rng(seed)
    pre = {}
    for name, s in shapes.items():
        p = R.spread(s, rng, -10, 30)
        empty = ref[name][2] == 0
        pat = np.where(np.arange(s[1]) % 2 == 0, NAN_PAYLOAD, NEG_ZERO).astype(np.uint32).view(np.float32)
        p[empty] = pat
        pre[name] = p
    assert (ref["dW"][2] == 0).any() and (ref["dP"][2] == 0).any()
    got = _emb_call(lib, c, t, H, S, n_types, drop_p, seed, pre)
    for name in shapes:
        tz, p, cnt = runs[0][name], pre[name], ref[name][2]
        _same(got[name][cnt == 0], p[cnt == 0], name + " untouched rows")
        touched = (cnt > 0)[:, None] & (tz != 0)                    # (a total of exactly zero is not added)
        _same(got[name][touched], _fl32_add(p, tz)[touched], name + " = fl32(p + t)")
        _same(got[name][(cnt > 0)[:, None] & (tz == 0)], p[(cnt > 0)[:, None] & (tz == 0)], name + " zero totals")


@pytest.mark.parametrize("packed", (False, True))
def test_embedding_bwd_ordered_ones_onto_two_to_the_24(lib, packed):
    H, S, n_types = 32, 8, 2
    c = _emb_case("runs", H, S, packed, n_types, 0.0, 5)
    c["dout"][:c["total"]] = 1.0
    ids_t = torch.from_numpy(c["ids"]).to(DEV)
    t = dict(ids=ids_t, order=torch.sort(ids_t, stable=True)[1], dout=_dev_bf16(c["dout"]), types=torch.from_numpy(c["types"]).to(DEV),
             cu=torch.from_numpy(c["cu"]).to(DEV) if packed else None)
    ref = R.embedding_reference(c["ids"], c["types"], c["dout"], c["keep"], 1.0, c["pos"], c["V"], c["P_rows"], n_types)
    pre = {"dW": np.full((c["V"], H), 2.0 ** 24, dtype=np.float32), "dP": np.full((c["P_rows"], H), 2.0 ** 24, dtype=np.float32),
           "dT": np.full((n_types, H), 2.0 ** 24, dtype=np.float32)}
    got = _emb_call(lib, c, t, H, S, n_types, 0.0, 5, pre)
    for name in pre:
        want = np.float32(2.0 ** 24) + ref[name][0].astype(np.float32)           # the counts: small integers, exact
        assert np.array_equal(got[name], want), name
    assert ref["dW"][0].max() == 2 * CHUNK + 1
