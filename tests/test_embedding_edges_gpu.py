"""The embedding family of csrc/embedding.hip (embedding_fwd_kernel dense and packed, embedding_bwd_kernel, embedding_bwd_pos_kernel,
dropout_kernel) and its fp32 twin (csrc/fp32_ops.hip) against the float64 reference, the per-element bounds and the host restatement of
the dropout bits of tests/embedding_ref.py (tests/test_embedding_ref_cpu.py shows what those bounds catch that max|a - r| / max|r| < 2e-2
lets through).  Every case runs through the C ABI with dW / dP / dT PRE-FILLED by a sentinel pattern (after - before is judged on touched
elements, bits on untouched ones; P has two rows more than S) and through K.embedding, whose fresh zero buffers give the gradient
bound its full sharpness.  Pass criterion: worst err / bound <= 1 for every quantity of every case;
nothing is excluded except rows that do not exist.

Shapes (sequences x S x H): 1 x 1 x 8, 37 x 8 x 8 (one slice, one partial column block); 37 x 8 x 264 (second column block, 8-wide tail);
37 x 16 x 768, 3 x 8 x 1024 (product widths); 257 x 8 x 264, 513 x 8 x 8 (2, 3 batch slices of the position kernel); 4097 x 8 x 264
(17 -> the cap of 16 slices, walkers stride 16).  A row index >= 2^32 (the high word of the row hash) is not reachable at test size: it
would need 2^32 rows of activations; the host restatement checks that word in test_embedding_ref_cpu.py instead.

Worst err / bound per kernel, family and quantity, measured on an MI355X ("abi": the C ABI onto the sentinel pre-fill, whose bound
carries the pre-filled value as one more term; "K": K.embedding onto zeros).  Dense rows take the worst over the small shapes, p = 0,
1e-6, 0.1, 0.5 and every types family.  The figures are the kernels as they stand; "before" (the kernels before this file existed)
differs in the abi columns only and only by "inf" = bits of an element without a term changed: dW in 41 of the 109 tests of this file
(every test that drops, has a zero element in a non-zero row, or runs the fp32 twin on zeros), dP in 7 and dT in 4 (fp32 twin only).

    bf16, dense sweep   out    dW abi (before) / K    dP abi / K     dT abi / K
    dout randn          0.25   0.50 (inf) / 0.51      0.30 / 0.30    0.30 / 0.30
    dout row_scaled     0.25   0.50 (inf) / 0.51      0.30 / 0.30    0.34 / 0.30
    dout sparse_rows    0.25   0.42 (inf) / 0.47      0.45 / 0.48    0.41 / 0.44
    dout cancel         0.25   0.41 (inf) / 0.47      0.30 / 0.30    0.30 / 0.30
    dout coded (p = 0)  0.25   0 (inf): torch.equal on every table, both entry points
    ids uniform         0.25   0.50 (inf) / 0.50      0.42 / 0.48    0.40 / 0.44
    ids zipf            0.25   0.46 (inf) / 0.51      0.45 / 0.45    0.41 / 0.42
    ids single          0.25   0.28 (inf) / 0.28      0.42 / 0.48    0.31 / 0.31
    ids distinct        0.25   0.41 (inf) / 0.41      0.45 / 0.45    0.41 / 0.36    (and dW rows bit-equal to keep o scale dout)

    bf16, zipf / row_scaled / 4 types / p = 0.1        out    dW abi (before) / K    dP abi / K     dT abi / K
    37 x 16 x 768                                      0.25   0.46 (inf) / 0.51      0.11 / 0.11    0.01 / 0.01
    3 x 8 x 1024                                       0.25   0.43 (inf) / 0.42      0.45 / 0.46    0.39 / 0.50
    257 x 8 x 264    (2 slices)                        0.25   0.41 (inf) / 0.41      0.01 / 0.01    0.00 / 0.00
    513 x 8 x 8      (3 slices)                        0.25   0.34 (inf) / 0.34      0.00 / 0.00    0.00 / 0.00
    4097 x 8 x 264   (16 slices, walkers stride 16)    0.25   0.39 (inf) / 0.41      0.00 / 0.00    0.00 / 0.00
    coded, skip_of_4, 257 x 8 x 264 and 4097 x 8 x 8   0.25   0 (inf at 257 x 8 x 264): torch.equal, every slice partial and atomic exact

    packed, p = 0 and 0.1   out    dW abi (before) / K    dP abi / K     dT abi / K     packed - dense (p = 0; 2 bounds)
    all 1, n = 1            0.19   0.18 (inf) / 0.41      0.18 / 0.41    0.27 / 0.41    0.00
    all 1, n = 257          0.25   0.43 (inf) / 0.47      0.00 / 0.00    0.03 / 0.03    0.00    (dP rows >= 1 bit-identical)
    all S, n = 64 (no tail) 0.25   0.32 (inf) / 0.38      0.02 / 0.02    0.01 / 0.01    0.00
    all S, n = 513          0.25   0.30 / 0.38            0.00 / 0.00    0.00 / 0.00    0.00
    ragged, n = 257         0.25   0.42 (inf) / 0.41      0.06 / 0.06    0.00 / 0.00    0.00
    ragged, n = 513         0.25   0.28 (inf) / 0.32      0.01 / 0.01    0.00 / 0.00    0.00
    holes, n = 37           0.25   0.51 (inf) / 0.51      0.20 / 0.24    0.03 / 0.04    0.01

    fp32 twin           out    dW abi (before) / K    dP abi (before) / K    dT abi (before) / K
    dout randn          0.03   0.21 / 0.04            0.04 / 0.01            0.01 / 0.00
    dout row_scaled     0.03   0.47 / 0.04            0.11 / 0.12            0.06 / 0.05
    dout sparse_rows    0.03   0.21 (inf) / 0.00      0.20 (inf) / 0.01      0.13 (inf) / 0.00
    dout cancel         0.03   0.21 / 0.04            0.04 / 0.01            0.02 / 0.00
    dout coded          0.03   0 (inf): torch.equal
    37 x 16 x 768       0.02   0.51 / 0.14            0.04 / 0.04            0.01 / 0.01
    3 x 8 x 1024        0.02   0.21 / 0.00            0.26 / 0.26            0.19 / 0.20
    257 x 8 x 264       0.02   0.31 / 0.01            0.01 / 0.00            0.00 / 0.00
    513 x 8 x 8         0.02   0.20 / 0.00            0.00 / 0.00            0.00 / 0.00

emdr2_dropout: bit-equal to the host mask and bf16(x * keep_scale_f32) at every cols, row count, p and seed (0 and 2^32 - 1).

The 0.25 of out is the bf16 store (half an ulp against C_BF16 = 2^-7 plus one ulp).  dW near 0.5 are elements of one or two terms
at p > 0: the fp32 keep scale and the product round once each, about 1.6 u against GRAD_WIDEN x 3 u.

What these tests found and what changed with them:
  * embedding_bwd_kernel added the +0.0 of every dropped element, and of every zero element of a non-zero row, to dW atomically, and
    emb_bwd_f32_kernel added every zero of dout to all three tables: x + (+0.0) is x for every x but -0.0, which becomes +0.0.  No sum
    changes, but "an element without a term keeps its previous contents bit for bit" did not hold for a -0.0 (the sentinel pre-fill
    has one in seven).  Both kernels now skip a zero term, as the position kernel always did (`if (ap != 0.f)`); the backward at the
    reader's shape (3,200 x 512 x 768, half padding, p = 0.1) went from 4.489 to 4.509 ms with it.
  * No wrong value.  The position kernel's 2, 3 and 16 slices, its second column block and 8-wide tail, 1 to 4 types and a type that
    never occurs, packed backward with dropout, a word row hit 16,000 times next to rows hit once, the zero-row skip on -0.0 rows, tail
    rows, P rows >= S and the fp32 twin all stay within their bounds, and the device mask is the host restatement bit for bit.
  * A flaw in tests/elementwise_ref.ln_bounds that only the fp32 constants expose is described in test_fp32_path_edges_gpu.py.
"""
import numpy as np
import pytest
import torch

from tests import embedding_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
SMALL = ((1, 1, 8), (37, 8, 8), (37, 8, 264))
LARGE = ((37, 16, 768), (3, 8, 1024), (257, 8, 264), (513, 8, 8), (4097, 8, 264))
PS = (0.0, 1e-6, 0.1, 0.5)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _nat():
    from emdr2_amd import _native
    return _native, _native.lib()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _merge(into, ratios, prefix=""):
    for n, (v, idx) in ratios.items():
        if not v <= into.get(prefix + n, (-1.0, None))[0]:
            into[prefix + n] = (v, idx)


def _assert(tag, ratios):
    print("[emb-edges] %s " % tag + " ".join("%s=%.3f" % (n, r[0]) for n, r in sorted(ratios.items())))
    bad = {n: r for n, r in ratios.items() if not r[0] <= 1.0}
    assert not bad, (tag, bad)


def _inputs(idfam, dfam, tfam, nseq, S, H, seed):
    g = _gen(seed)
    n = nseq * S
    V = E.vocab_for(idfam, n)
    ids = E.ids_inputs(idfam, n, V, g, DEV)
    types, nt = E.types_inputs(tfam, n, g, DEV)
    W, P, T = E.tables(V, S + 2, nt, H, g, DEV)
    return ids.reshape(nseq, S), types, nt, W, P, T, E.dout_inputs(dfam, ids, H, g, DEV)


def _prefill(W, P, T):
    before = {"dW": E.sentinel(W.shape, DEV), "dP": E.sentinel(P.shape, DEV)}
    if T is not None:
        before["dT"] = E.sentinel(T.shape, DEV)
    return before


def _abi_dense(ids, types, nt, W, P, T, dout, p, seed, before):
    """emdr2_embedding_fwd + emdr2_embedding_bwd on bf16 tables / dout, accumulating into copies of `before`."""
    nat, lib = _nat()
    nseq, S = ids.shape
    H = W.shape[1]
    Wb, Pb, Tb = W.to(BF16), P.to(BF16), (None if T is None else T.to(BF16))
    out = torch.full((nseq * S, H), float("nan"), dtype=BF16, device=DEV)
    nat.check(lib.emdr2_embedding_fwd(ids.data_ptr(), _ptr(types), Wb.data_ptr(), Pb.data_ptr(), _ptr(Tb), out.data_ptr(), nseq * S, S, H, float(p),
                                      int(seed), nat.stream_ptr()), "embedding_fwd")
    got = {k: v.clone() for k, v in before.items()}
    db = dout.to(BF16).contiguous()
    nat.check(lib.emdr2_embedding_bwd(ids.data_ptr(), _ptr(types), db.data_ptr(), got["dW"].data_ptr(), got["dP"].data_ptr(), _ptr(got.get("dT")),
                                      nseq * S, S, H, nt, float(p), int(seed), nat.stream_ptr()), "embedding_bwd")
    torch.cuda.synchronize()
    got["out"] = out
    return got


def _wrapper(ids, types, W, P, T, dout, p, seed, seqs=None, fp32=False):
    """K.embedding forward + backward on fresh parameters -> out, dW, dP (+ dT) (the gradients start from zero)."""
    from emdr2_amd.model import kernels as K
    Wp, Pp = torch.nn.Parameter(W.clone()), torch.nn.Parameter(P.clone())
    Tp = None if T is None else torch.nn.Parameter(T.clone())
    if seqs is not None:
        out = K.embedding(None, None, Wp, Pp, Tp, p, seed, seqs=seqs)
    else:
        out = K.embedding(ids, None if T is None else types.reshape(ids.shape), Wp, Pp, Tp, p, seed, fp32=fp32)
    out.backward((dout if fp32 else dout.to(BF16)).reshape(out.shape))
    torch.cuda.synchronize()
    got = {"out": out.detach().reshape(-1, W.shape[1]), "dW": Wp.grad, "dP": Pp.grad}
    if Tp is not None:
        got["dT"] = Tp.grad
    return got


def _zeros_like(before):
    return {k: torch.zeros_like(v) for k, v in before.items()}


def _forward_checks(tag, r, out, W, P, T, p, fp32=False):
    """The zero pattern is the keep bits exactly (+0 at dropped elements and tail rows); at p = 0 the bits are ((W + P) + T) in fp32."""
    bits = out.view(torch.int32 if fp32 else torch.int16)
    assert bool((bits[~r.kept] == 0).all()), (tag, "a dropped element or a tail row is not +0")
    assert torch.equal(out != 0, r.kept & (r.out != 0)), (tag, "the forward's zero pattern differs from keep_bits")
    if not p > 0.0:
        v = W.float()[r.ids] + P.float()[r.pos]
        if r.types is not None:
            v = v + T.float()[r.types]
        v = torch.where(r.kept, v, torch.zeros_like(v))
        assert bool(E.same_bits(out, v if fp32 else v.to(BF16)).all()), (tag, "p = 0: the forward is not ((W + P) + T) to the bit")


def _judge(tag, r, got, before, W, P, T, p, fp32=False, exact=False, distinct_scale=None):
    B = E.embedding_bounds(r, *((E.C_F32, 23) if fp32 else (E.C_BF16, 7)))
    ratios = {"out": E.worst(got["out"], r.out, B["out"])}
    _forward_checks(tag, r, got["out"], W, P, T, p, fp32)
    ratios.update(E.worst_grads(got, before, r, B))
    if exact:                                                            # the coded family: fp32 sums of small integers, any order
        for n in before:
            assert torch.equal(got[n].double(), before[n].double() + getattr(r, n)), (tag, n, "exact family")
    if distinct_scale is not None:                                       # no id twice: dW rows are keep o scale dout, one fp32 add each
        term = torch.where(r.kept, r.dout.float() * torch.tensor(distinct_scale, dtype=torch.float32, device=DEV), torch.zeros_like(r.dout.float()))
        assert torch.equal(got["dW"][r.ids], before["dW"][r.ids] + term), (tag, "distinct ids: dW rows are not keep o scale dout")
    return ratios


def _dense_case(idfam, dfam, tfam, nseq, S, H, p, seed, wrapper):
    ids, types, nt, W, P, T, dout = _inputs(idfam, dfam, tfam, nseq, S, H, seed)
    keep = E.keep_bits(nseq * S, H, p, seed, DEV) if p > 0 else None
    r = E.embedding_reference(ids, types, W, P, T, keep, E.keep_scale_exact(p) if p > 0 else 1.0, dout)
    tag = "%s/%s/%s %dx%dx%d p=%g" % (idfam, dfam, tfam, nseq, S, H, p)
    before = _prefill(W, P, T)
    exact = dfam == "coded"
    sc = (E.keep_scale_f32(p) if p > 0 else 1.0) if idfam == "distinct" else None
    ratios = {}
    _merge(ratios, _judge(tag + " abi", r, _abi_dense(ids, types, nt, W, P, T, dout, p, seed, before), before, W, P, T, p, exact=exact,
                          distinct_scale=sc))
    if wrapper:
        zero = _zeros_like(before)
        _merge(ratios, _judge(tag + " K.embedding", r, _wrapper(ids, types, W, P, T, dout, p, seed), zero, W, P, T, p, exact=exact,
                              distinct_scale=sc), "K_")
    return tag, ratios


# ---- the dense sweep: ids x dout x types families at every p, on the small shapes ---------------------------------------------------------
@pytest.mark.parametrize("idfam", E.IDS_FAMILIES)
@pytest.mark.parametrize("p", PS)
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "%dx%dx%d" % s)
def test_dense_sweep(shape, p, idfam):
    nseq, S, H = shape
    for dfam in E.DOUT_FAMILIES + (E.EXACT_DOUT_FAMILIES if p == 0.0 else ()):
        ratios = {}
        for tfam in E.TYPES_FAMILIES:
            _, one = _dense_case(idfam, dfam, tfam, nseq, S, H, p, 0x51 + H, True)
            _merge(ratios, one)
        _assert("dense %s/%s %dx%dx%d p=%g" % (idfam, dfam, nseq, S, H, p), ratios)


@pytest.mark.parametrize("shape", LARGE, ids=lambda s: "%dx%dx%d" % s)
def test_dense_large_shapes(shape):
    """Product widths, 2 and 3 batch slices of the position kernel and its cap of 16: zipf ids, row_scaled dout, four types, p = 0.1."""
    nseq, S, H = shape
    tag, ratios = _dense_case("zipf", "row_scaled", "t4", nseq, S, H, 0.1, 0xBEEF01, True)
    _assert("large " + tag, ratios)


@pytest.mark.parametrize("shape", ((257, 8, 264), (4097, 8, 8)), ids=lambda s: "%dx%dx%d" % s)
def test_dense_slices_exact(shape):
    """The coded family across 2 and 16 slices: every slice partial and every atomic is exact, so a lost or doubled slice is a bit error."""
    nseq, S, H = shape
    tag, ratios = _dense_case("zipf", "coded", "skip_of_4", nseq, S, H, 0.0, 5, True)
    _assert("slices-exact " + tag, ratios)


# ---- the packed layout ---------------------------------------------------------------------------------------------------------------------
def _lengths(fam, n, S):
    a = np.arange(n)
    if fam == "all1":
        return np.ones(n, dtype=np.int64)
    if fam == "allS":
        return np.full(n, S, dtype=np.int64)
    return (1 + (a * 5 + 2) % S).astype(np.int64)                        # ragged: 1 .. S


PACKED_CASES = [("all1", 1, 8), ("all1", 257, 264), ("allS", 64, 8), ("allS", 513, 8), ("ragged", 257, 264), ("ragged", 513, 8), ("holes", 37, 264)]


@pytest.mark.parametrize("p", (0.0, 0.1))
@pytest.mark.parametrize("lfam,n,H", PACKED_CASES)
def test_packed(lfam, n, H, p):
    """PackedSeqs layouts: all lengths 1 (only position 0 exists: dP rows >= 1 untouched), all S (64 x 8 = 512 rows: no tail; 513 x 8: a
    tail), ragged, and `holes` = ragged with one all-pad sequence (it keeps S rows of id 0) and zeros inside sequences.  Against the
    float64 reference; at p = 0 against the dense launch at the real positions (the mask of a packed row is that of its PACKED row
    index, so with dropout the two layouts draw different bits); tail rows of out are +0; tail rows of dout are +0.0 and -0.0 rows and
    add nothing (the contract of the kernel: "a tail row carries a zero gradient")."""
    from emdr2_amd.model import kernels as K
    S, seed = 8, 0x51 + n
    g = _gen(seed)
    lens = torch.from_numpy(_lengths("ragged" if lfam == "holes" else lfam, n, S)).to(DEV)
    V = 64
    ids = E.ids_inputs("zipf", n * S, V, g, DEV, lo=1).reshape(n, S)
    ids = torch.where(torch.arange(S, device=DEV)[None] < lens[:, None], ids, torch.zeros_like(ids))
    if lfam == "holes":
        ids[3] = 0                                                       # all pad: the layout keeps its S rows
        lens[3] = S
        ids[5, 0] = 0                                                    # zeros inside: sequence 5 (length 4) starts with one,
        ids[7, 1] = 0                                                    # sequence 7 (length 6) has one at position 1
    types, nt = E.types_inputs("t4", n * S, g, DEV)
    seqs = K.PackedSeqs(ids, types.reshape(n, S))
    cu = seqs.cu.long()
    assert torch.equal(cu[1:] - cu[:-1], lens), "the layout's lengths are not the ones this test planted"
    rows, total = seqs.rows, seqs.total
    assert (rows == total) == (lfam == "allS" and n == 64)
    W, P, T = E.tables(V, S + 2, nt, H, g, DEV)
    dout = torch.zeros((rows, H), device=DEV)
    dout[:total] = E.dout_inputs("row_scaled", seqs.ids[:total], H, g, DEV)
    dout[total::2] = -0.0                                                # tail rows: -0.0 and +0.0 rows alternate
    keep = E.keep_bits(rows, H, p, seed, DEV) if p > 0 else None
    r = E.embedding_reference(seqs.ids, seqs.types, W, P, T, keep, E.keep_scale_exact(p) if p > 0 else 1.0, dout, S=S, cu=seqs.cu, rowmap=seqs.rowmap)
    tag = "packed %s n=%d H=%d p=%g (%d of %d rows real)" % (lfam, n, H, p, total, rows)
    # C ABI onto sentinels
    nat, lib = _nat()
    before = _prefill(W, P, T)
    Wb, Pb, Tb = W.to(BF16), P.to(BF16), T.to(BF16)
    out = torch.full((rows, H), float("nan"), dtype=BF16, device=DEV)
    nat.check(lib.emdr2_embedding_packed_fwd(seqs.ids.data_ptr(), seqs.types.data_ptr(), seqs.rowmap.data_ptr(), Wb.data_ptr(), Pb.data_ptr(), Tb.data_ptr(),
                                             out.data_ptr(), rows, S, H, float(p), seed, nat.stream_ptr()), "embedding_packed_fwd")
    got = {k: v.clone() for k, v in before.items()}
    db = dout.to(BF16)
    nat.check(lib.emdr2_embedding_packed_bwd(seqs.ids.data_ptr(), seqs.types.data_ptr(), seqs.cu.data_ptr(), n, db.data_ptr(), got["dW"].data_ptr(),
                                             got["dP"].data_ptr(), got["dT"].data_ptr(), rows, S, H, nt, float(p), seed, nat.stream_ptr()),
              "embedding_packed_bwd")
    torch.cuda.synchronize()
    got["out"] = out
    ratios = {}
    _merge(ratios, _judge(tag + " abi", r, got, before, W, P, T, p))
    zero = _zeros_like(before)
    gw = _wrapper(None, None, W, P, T, dout, p, seed, seqs=seqs)
    _merge(ratios, _judge(tag + " K.embedding", r, gw, zero, W, P, T, p), "K_")
    assert bool((out[total:].view(torch.int16) == 0).all())
    if lfam == "all1":
        assert bool(E.same_bits(got["dP"][1:], before["dP"][1:]).all()) and float(r.aP[1:].max()) == 0.0
    if not p > 0.0:                                                      # the dense launch of the same grid
        real = seqs.rowmap[:total].long()
        dd = torch.zeros((n * S, H), device=DEV)
        dd[real] = dout[:total]
        gd = _wrapper(ids, types, W, P, T, dd, 0.0, seed)
        assert torch.equal(gd["out"][real].view(torch.int16), gw["out"][:total].view(torch.int16)), (tag, "packed forward differs from the dense one")
        Bd = E.embedding_bounds(r)
        for name in ("dW", "dP", "dT"):                                  # both lie within one bound of the same sums
            ratios["dense_" + name] = E.worst(gw[name], gd[name].double(), 2.0 * Bd[name])
    _assert(tag, ratios)


# ---- emdr2_dropout -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", (0, 2 ** 32 - 1))
@pytest.mark.parametrize("p", (0.1, 0.5))
@pytest.mark.parametrize("rows", (1, 37))
@pytest.mark.parametrize("cols", (8, 264, 768))
def test_dropout_kernel_is_the_host_mask(cols, rows, p, seed):
    """The mask of emdr2_dropout is keep_bits; survivors are bf16(x * keep_scale_f32), dropped elements +0."""
    nat, lib = _nat()
    x = torch.randn((rows, cols), generator=_gen(cols + rows), device=DEV).to(BF16)
    x[0, :4] = torch.tensor([0.0, -0.0, 2.0 ** -120, -3.0e38], device=DEV).to(BF16)
    out = torch.full_like(x, float("nan"))
    nat.check(lib.emdr2_dropout(x.data_ptr(), out.data_ptr(), x.numel(), cols, p, seed, nat.stream_ptr()), "dropout")
    torch.cuda.synchronize()
    keep = E.keep_bits(rows, cols, p, seed, DEV)
    want = (x.float() * torch.tensor(E.keep_scale_f32(p), dtype=torch.float32, device=DEV)).to(BF16)
    want = torch.where(keep, want, torch.zeros_like(want))
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))


# ---- the fp32 twin -------------------------------------------------------------------------------------------------------------------------
def _f32_case(idfam, dfam, tfam, nseq, S, H, seed, wrapper):
    nat, lib = _nat()
    ids, types, nt, W, P, T, dout = _inputs(idfam, dfam, tfam, nseq, S, H, seed)
    g = _gen(seed + 1)
    W = W + 2.0 ** -12 * torch.randn(W.shape, generator=g, device=DEV)     # fp32 tables as they are: not bf16 values
    P = P + 2.0 ** -12 * torch.randn(P.shape, generator=g, device=DEV)
    r = E.embedding_reference(ids, types, W, P, T, None, 1.0, dout)
    tag = "f32 %s/%s/%s %dx%dx%d" % (idfam, dfam, tfam, nseq, S, H)
    before = _prefill(W, P, T)
    out = torch.full((nseq * S, H), float("nan"), device=DEV)
    nat.check(lib.emdr2_f32_embedding_fwd(ids.data_ptr(), _ptr(types), W.data_ptr(), P.data_ptr(), _ptr(T), out.data_ptr(), nseq * S, S, H, nat.stream_ptr()),
              "f32_embedding_fwd")
    got = {k: v.clone() for k, v in before.items()}
    nat.check(lib.emdr2_f32_embedding_bwd(ids.data_ptr(), _ptr(types), dout.data_ptr(), got["dW"].data_ptr(), got["dP"].data_ptr(), _ptr(got.get("dT")),
                                          nseq * S, S, H, nat.stream_ptr()), "f32_embedding_bwd")
    torch.cuda.synchronize()
    got["out"] = out
    ratios = {}
    _merge(ratios, _judge(tag + " abi", r, got, before, W, P, T, 0.0, fp32=True, exact=dfam == "coded", distinct_scale=1.0 if idfam == "distinct" else None))
    if wrapper:
        _merge(ratios, _judge(tag + " K.embedding", r, _wrapper(ids, types, W, P, T, dout, 0.0, 0, fp32=True), _zeros_like(before), W, P, T, 0.0, fp32=True,
                              exact=dfam == "coded"), "K_")
    return tag, ratios


@pytest.mark.parametrize("idfam", E.IDS_FAMILIES)
@pytest.mark.parametrize("shape", SMALL, ids=lambda s: "%dx%dx%d" % s)
def test_f32_twin_sweep(shape, idfam):
    nseq, S, H = shape
    for dfam in E.DOUT_FAMILIES + E.EXACT_DOUT_FAMILIES:
        ratios = {}
        for tfam in E.TYPES_FAMILIES:
            _, one = _f32_case(idfam, dfam, tfam, nseq, S, H, 0x51 + H, True)
            _merge(ratios, one)
        _assert("f32 %s/%s %dx%dx%d" % (idfam, dfam, nseq, S, H), ratios)


@pytest.mark.parametrize("shape", LARGE[:4], ids=lambda s: "%dx%dx%d" % s)
def test_f32_twin_large_shapes(shape):
    nseq, S, H = shape
    tag, ratios = _f32_case("zipf", "row_scaled", "t4", nseq, S, H, 0xBEEF01, True)
    _assert("large " + tag, ratios)
