"""Attention kernels against a float64 reference with ROW-SCALED bounds: score range, mask patterns, every launch path.

Every case goes through K.attention_core (the product's dispatch: dense fused kernels, emdr2_attention_varlen_* for packed operands,
emdr2_attention_*_splitkv for long keys, the GEMM + softmax_mask_* composition for head dims other than 64, kernels_f32 for fp32 operands)
and checks O, dQ, dK, dV and the saved statistics m + ln l against tests/attention_ref.py: bounds, input families and mask patterns are
described there; tests/test_attention_ref_cpu.py shows that these bounds catch planted faults which the whole-tensor metric
max|a - r| / max|r| passes.  Nothing is excluded but rows that do not exist (the tail rows of a packed layout, which must stay zero).

Worst err / bound per case family, measured on the kernels as they stood before this file existed (c = 2^-7; fp32 path c = 2^-18):

    family / path                      O      dQ      dK      dV     lse  uniform (rows vs mean V)
    fused  randn                    0.45    0.17    0.29    0.37    0.06    0.32
    fused  stair_up                 0.45    0.21    0.24    0.37    0.07    0.39
    fused  stair_under              0.49    0.18    0.28    0.42    0.09    0.38
    fused  stair_mixed              0.42    0.21    0.35    0.43    0.11    0.30
    fused  one_hot                  0.47    0.36    0.41    0.49    0.16    0.41
    fused  flat                     0.43    0.18    0.26    0.36    0.06    0.40
    fused  dropout randn            0.20    0.17    0.24    0.28    0.06       -
    fused  dropout stair_up         0.24    0.17    0.14    0.24    0.06       -
    fused  masks randn              0.46    0.20    0.34   83.06    0.07    0.28      dV: causal_key0 (0.40 with the fix below)
    fused  masks stair_up           0.42    0.21    0.32   81.39    0.10    0.28      dV: causal_key0 (0.41 with the fix below)
    split  randn                    0.06    0.07    0.37    0.40    0.06    0.03
    split  stair_up                 0.15    0.15    0.24    0.27    0.06    0.03
    split  packed grouped keys      0.48    0.16    0.38    0.37    0.06       -
    packed self-attention           0.45    0.21    0.31    0.44    0.12       -
    composed hn32 randn             0.43    0.27    0.36    0.45    0.78    0.17
    composed hn32 stair_up          0.43    0.26    0.62    0.48    0.66    0.17
    composed hn16 randn             0.41    0.30    0.43    0.43    0.83    0.18      (hn = 16 and sq % 32 != 0 did not run before: see below)
    composed hn16 stair_up          0.44    0.31    0.87    0.57    0.70    0.18
    fp32   masks randn              0.03    0.01    0.01    0.03  P 0.01    0.03
    fp32   masks stair_up           0.05    0.02    0.17    0.16  P 0.12    0.03

The fused O column sits at 0.4 - 0.5 on every family: the bf16 store of a causal row with one or two visible keys, whose own rounding
(up to 2^-8 of the value) is half of c by itself.  Composed lse 0.7 - 0.8: a causal row 0 has lse = s_00, stored in bf16 at that format's
unit roundoff; composed dK / dV on the staircase: dP and dS are stored in bf16 there, two roundings more than the fused kernels make.
Without the underflow term of attention_ref.py the 4,160-key staircase read dK 57, dV 59 (absolute errors of 1e-38); without the fp32
score term the fp32 staircase read O 2.3, dQ 1.6, dV 1.5.

What these tests found and what changed with them:
  * causal_key0 (a real query whose only visible key is padding: its row is uniform over ALL keys) and, with it, every padded query of a
    causal launch: the dK / dV kernel skipped the key waves ahead of the query step, so those keys' dV missed the row's dO / sk
    (dV 83 bounds off at key 95; both families).  attention_bwd.hip keeps such a step now.
  * the composition rejected head dims and query counts that are no multiple of 32 (its GEMMs' contraction length): it pads them now.
"""
import pytest
import torch

from tests import attention_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _drop_mask(b, heads, sq, sk, p, seed):
    """The site's keep pattern through the kernel the other dropout tests use, scaled by the exact 1 / (1 - p) of csrc/rng.h
    (the bf16 ones that kernel scales would carry a rounding of their own into the reference)."""
    from tests.test_ops_gpu import _dropout_mask
    return (_dropout_mask((b, heads, sq, sk), p, seed) != 0).double() * R.keep_scale(p)


def _launch(q, k, v, dO, ids_q, ids_k, causal, drop_p=0.0, seed=0, fp32=False, self_layout=False):
    """q [b, sq, n, hn], k / v [b, sk, n, hn], dO: fp32 tensors holding bf16 values -> dict O, dQ, dK, dV, saved (m, l | P)."""
    from emdr2_amd.model import kernels as K
    dt = torch.float32 if fp32 else torch.bfloat16
    if self_layout:                                                      # self-attention: ONE packed [b, s, 3, n, hn] projection output
        qkv = torch.stack([q, k, v], dim=2).to(dt).requires_grad_(True)
        out = K.attention_core(qkv, None, ids_q, ids_k, causal, drop_p=drop_p, seed=seed)
    else:
        qq = q.to(dt).clone().requires_grad_(True)
        kv = torch.stack([k, v], dim=2).to(dt).requires_grad_(True)
        out = K.attention_core(qq, kv, ids_q, ids_k, causal, drop_p=drop_p, seed=seed)
    saved = tuple(t.detach().clone() for t in out.grad_fn.saved_tensors[2:])
    out.backward(dO.to(dt))
    torch.cuda.synchronize()
    if self_layout:
        g = qkv.grad
        return {"O": out.detach(), "dQ": g[:, :, 0], "dK": g[:, :, 1], "dV": g[:, :, 2], "saved": saved}
    return {"O": out.detach(), "dQ": qq.grad, "dK": kv.grad[:, :, 0], "dV": kv.grad[:, :, 1], "saved": saved}


def _ratios(got, ref, c=R.C_BF16, score_round=0.0, mant_bits=7, stats=True, v=None, score_abs=False):
    """Worst err / bound of every checked quantity -> {name: (ratio, index)}."""
    B = R.bounds(ref, c, score_round, mant_bits, score_abs)
    out = {name: R.worst(got[name], getattr(ref, name), B[name]) for name in ("O", "dQ", "dK", "dV") if name in got}
    if stats:
        m, l = got["saved"][0].double(), got["saved"][1].double()
        out["lse"] = R.worst(m + torch.log(l), ref.lse, R.lse_bound(ref, score_round))
    if v is not None:                                                    # rows the reference makes uniform: directly against mean(V) over all sk keys
        out["uniform"] = (R.worst_uniform(got["O"], v, ref, c), ())
    return out


def _assert(tag, ratios):
    print("[attn-edges] %s " % tag + " ".join("%s=%.3f" % (n, r[0]) for n, r in ratios.items()))
    bad = {n: r for n, r in ratios.items() if not r[0] < 1.0}
    assert not bad, (tag, bad)


def _dense_case(tag, fam, pattern, b, heads, sq, sk, causal, hn=64, drop_p=0.0, fp32=False, seed=0, pos_k=None, ids=None):
    q, k, v, dO = R.family(fam, b, heads, sq, sk, hn, _gen(seed + 11), DEV, pos_k)
    ids_q, ids_k = ids if ids is not None else R.mask_ids(pattern, b, sq, sk, DEV)
    dseed = 0xA77E + seed
    # (the composition pads its query grid to whole 32-row steps: its dropout rows and statistics are those of the padded grid)
    sp = sq if hn == 64 or fp32 else (sq + 31) // 32 * 32
    mask = _drop_mask(b, heads, sp, sk, drop_p, dseed)[:, :, :sq] if drop_p > 0 else None
    got = _launch(q, k, v, dO, ids_q, ids_k, causal, drop_p, dseed, fp32, self_layout=(sq == sk and hn == 64))
    ref = R.reference(q, k, v, ids_q, ids_k, causal, mask, dO)
    if fp32:                                                             # fp32 scores: the hn-term dot product's own error (attention_ref.py)
        sr = 2.0 * hn * 2.0 ** -24
        ratios = _ratios(got, ref, R.C_F32, sr, 23, stats=False, v=v, score_abs=True)
        ratios["P"] = R.worst(got["saved"][0], ref.P, R.p_bound(ref, R.C_F32, sr, True))     # this path keeps the probabilities, not (m, l)
    else:
        composed = hn != 64
        got["saved"] = tuple(t[..., :sq] for t in got["saved"][:2])
        ratios = _ratios(got, ref, R.C_BF16, 2.0 ** -8 if composed else 0.0, 7, True, v if drop_p == 0 else None)
    _assert(tag, ratios)
    return got, ref


# ---- score range: the families at the dense and causal shapes --------------------------------------------------------------------
@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("shape", [(2, 2, 64, 256, False), (2, 2, 96, 96, True), (2, 2, 32, 32, True)], ids=["dense", "causal96", "causal32"])
def test_score_range_families(fam, shape):
    b, heads, sq, sk, causal = shape
    _dense_case("fused/%s/%dx%d" % (fam, sq, sk), fam, "trailing", b, heads, sq, sk, causal, seed=R.FAMILIES.index(fam))


@pytest.mark.parametrize("fam", ["randn", "stair_up"])
def test_score_range_with_dropout(fam):
    _dense_case("fused-drop/%s" % fam, fam, "trailing", 2, 2, 64, 256, False, drop_p=0.1, seed=3)


# ---- mask patterns ------------------------------------------------------------------------------------------------------------------
def _pattern_shape(pat):
    if pat == "causal_key0":
        return 96, 96, True
    return (64, 192, False) if pat == "all_keys" else (64, 256, False)


@pytest.mark.parametrize("fam", ["randn", "stair_up"])
@pytest.mark.parametrize("pat", R.MASK_PATTERNS)
def test_mask_patterns(fam, pat):
    sq, sk, causal = _pattern_shape(pat)
    _dense_case("fused-mask/%s/%s" % (pat, fam), fam, pat, 2, 2, sq, sk, causal, seed=20 + R.MASK_PATTERNS.index(pat))


@pytest.mark.parametrize("fam", ["randn", "stair_up"])
@pytest.mark.parametrize("pat", R.MASK_PATTERNS)
def test_mask_patterns_fp32_validation_path(fam, pat):
    sq, sk, causal = _pattern_shape(pat)
    _dense_case("fp32-mask/%s/%s" % (pat, fam), fam, pat, 2, 2, sq, sk, causal, fp32=True, seed=40 + R.MASK_PATTERNS.index(pat))


# ---- split-key launches -----------------------------------------------------------------------------------------------------------
SPLIT = (2, 1, 32, 4160)                                                  # 65 key blocks: three ranges of 32, 32 and 1


def _split_ids(pat):
    b, heads, sq, sk = SPLIT
    ids_q = torch.full((b, sq), 7, dtype=torch.int64, device=DEV)
    ids_k = torch.full((b, sk), 7, dtype=torch.int64, device=DEV)
    ids_k[1, sk - 5:] = 0
    ids_q[1, sq - 1:] = 0
    if pat == "first_split":
        ids_k[0, :2048] = 0
    elif pat == "middle_split":
        ids_k[0, 2048:4096] = 0
    elif pat == "all_keys":
        ids_k[0, :] = 0
    return ids_q, ids_k


@pytest.mark.parametrize("fam", ["randn", "stair_up"])
@pytest.mark.parametrize("pat", ["first_split", "middle_split", "all_keys", "trailing"])
def test_split_key_launches(fam, pat):
    """The staircase rises by 6 every 256 keys (8 rises inside a range, every range starts above the last one's end)."""
    from emdr2_amd.model import kernels as K
    b, heads, sq, sk = SPLIT
    assert K._splitkv_plan(b, heads, sq, sk)[0] > 1
    pos = (torch.arange(sk, device=DEV) // 8)[None].expand(b, sk)
    _dense_case("split/%s/%s" % (pat, fam), fam, None, b, heads, sq, sk, False, seed=60, pos_k=pos, ids=_split_ids(pat))


def _check_seqs(tag, got_seqs, refs, saved_seqs):
    """Per-sequence results of a packed launch: worst ratio over the sequences."""
    worst = {}
    for got, ref, (m, l) in zip(got_seqs, refs, saved_seqs):
        got = dict(got, saved=(m, l))
        for n, r in _ratios(got, ref).items():
            if n not in worst or r[0] > worst[n][0]:
                worst[n] = r
    _assert(tag, worst)


@pytest.mark.parametrize("fam", ["randn", "stair_up"])
def test_split_key_launch_over_packed_grouped_keys(fam):
    """Dense decoder queries over PackedSeqs.grouped keys: question 0 owns 4,224 keys (66 blocks, three ranges), question 1 three keys in
    all (two of its three ranges are empty); a padded query is uniform over its question's own keys."""
    from emdr2_amd.model import kernels as K
    B, Kk, S, L, heads = 2, 3, 1408, 32, 1
    ids = torch.zeros((B * Kk, S), dtype=torch.int64, device=DEV)
    ids[:Kk] = 7
    ids[Kk:, 0] = 7
    seqs = K.PackedSeqs(ids)
    gk = seqs.grouped(Kk)
    assert K._splitkv_plan(B, heads, L, gk.max_len)[0] > 1
    lens = [Kk * S, Kk]
    g = _gen(71)
    parts = [R.family(fam, 1, heads, L, n, 64, g, DEV, (torch.arange(n, device=DEV) // 8)[None]) for n in lens]
    q = torch.cat([p[0] for p in parts]).bfloat16().requires_grad_(True)
    dO = torch.cat([p[3] for p in parts])
    kv_rows = torch.zeros((seqs.rows, 2, heads, 64), device=DEV)
    kv_rows[:seqs.total, 0] = torch.cat([p[1][0] for p in parts])
    kv_rows[:seqs.total, 1] = torch.cat([p[2][0] for p in parts])
    kv = kv_rows.bfloat16().requires_grad_(True)
    dec = torch.full((B, L), 7, dtype=torch.int64, device=DEV)
    dec[0, L - 1] = 0
    dec[1, L - 2:] = 0
    out = K.attention_core(q, kv, dec, gk, False)
    m, l = (t.detach().clone() for t in out.grad_fn.saved_tensors[2:4])
    out.backward(dO.bfloat16())
    torch.cuda.synchronize()
    refs = R.reference_packed([p[0][0] for p in parts], [p[1][0] for p in parts], [p[2][0] for p in parts], False,
                              [p[3][0] for p in parts], [dec[0], dec[1]])
    cu = [0, lens[0], lens[0] + lens[1]]
    gots = [{"O": out.detach()[i][None], "dQ": q.grad[i][None], "dK": kv.grad[cu[i]:cu[i + 1], 0][None], "dV": kv.grad[cu[i]:cu[i + 1], 1][None]}
            for i in range(B)]
    _check_seqs("split-packed/%s" % fam, gots, refs, [(m[i][None], l[i][None]) for i in range(B)])
    assert float(kv.grad[seqs.total:].float().abs().max()) == 0.0         # rows that do not exist


# ---- packed self-attention ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("causal", [False, True])
def test_packed_self_attention_staircase(causal):
    from emdr2_amd.model import kernels as K
    lens, heads = [1, 33, 65, 130], 2
    ids = torch.zeros((len(lens), max(lens)), dtype=torch.int64, device=DEV)
    for i, n in enumerate(lens):
        ids[i, :n] = 7
    seqs = K.PackedSeqs(ids)
    g = _gen(81)
    parts = [R.family("stair_up", 1, heads, n, n, 64, g, DEV) for n in lens]
    rows = torch.zeros((seqs.rows, 3, heads, 64), device=DEV)
    for j in range(3):
        rows[:seqs.total, j] = torch.cat([p[j][0] for p in parts])
    qkv = rows.bfloat16().requires_grad_(True)
    dO = torch.zeros((seqs.rows, heads, 64), device=DEV)
    dO[:seqs.total] = torch.cat([p[3][0] for p in parts])
    out = K.attention_core(qkv, None, seqs, seqs, causal)
    m, l = (t.detach().clone() for t in out.grad_fn.saved_tensors[2:4])   # [heads, rows]
    out.backward(dO.bfloat16())
    torch.cuda.synchronize()
    refs = R.reference_packed([p[0][0] for p in parts], [p[1][0] for p in parts], [p[2][0] for p in parts], causal, [p[3][0] for p in parts])
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    sl = [slice(cu[i], cu[i + 1]) for i in range(len(lens))]
    gots = [{"O": out.detach()[s][None], "dQ": qkv.grad[s, 0][None], "dK": qkv.grad[s, 1][None], "dV": qkv.grad[s, 2][None]} for s in sl]
    _check_seqs("packed-self/causal=%d" % causal, gots, refs, [(m[:, s][None], l[:, s][None]) for s in sl])
    if seqs.rows > seqs.total:                                            # rows that do not exist stay exactly zero
        assert float(out.detach()[seqs.total:].float().abs().max()) == 0.0 and float(qkv.grad[seqs.total:].float().abs().max()) == 0.0


# ---- the GEMM + softmax composition (head dims other than 64) ---------------------------------------------------------------------
# The first three shapes have query counts that are no multiple of 32 (and hn = 16 is no multiple of 32 either): the composition runs
# them zero-padded; the last three run as they are.
COMPOSED_SHAPES = [(2, 2, 48, 64, False), (3, 2, 40, 160, False), (2, 3, 8, 32, True), (2, 2, 32, 64, False), (3, 2, 64, 160, False), (2, 3, 32, 32, True)]


@pytest.mark.parametrize("drop_p", [0.0, 0.1])
@pytest.mark.parametrize("fam", ["randn", "stair_up"])
@pytest.mark.parametrize("pat", ["trailing", "lead32", "all_keys"])
@pytest.mark.parametrize("shape", COMPOSED_SHAPES, ids=["%dx%d%s" % (s[2], s[3], "causal" if s[4] else "") for s in COMPOSED_SHAPES])
@pytest.mark.parametrize("hn", [16, 32])
def test_composed_path(hn, shape, pat, fam, drop_p):
    """Scores are stored in bf16 here: one more rounding inside the exponent, carried by the majorants as its own term
    (tests/attention_ref.py: score_round); c stays 2^-7."""
    b, heads, sq, sk, causal = shape
    _dense_case("composed/hn%d/%dx%d/%s/%s/p%.1f" % (hn, sq, sk, pat, fam, drop_p), fam, pat, b, heads, sq, sk, causal, hn=hn, drop_p=drop_p,
                seed=90 + hn)
