"""Float64 reference, per-element bounds, input families and a host restatement of the dropout bits for the embedding kernels of
csrc/embedding.hip (embedding_fwd_kernel dense and packed, embedding_bwd_kernel, embedding_bwd_pos_kernel), dropout_kernel (csrc/elementwise.hip) and their
fp32 twins in csrc/fp32_ops.hip -- CPU and GPU tensors alike.  The pattern is that of tests/attention_ref.py, tests/elementwise_ref.py and
tests/gemm_ref.py, whose constants are imported, not restated.

The op (language_model.py:169-181):  out[t] = keep[t] o scale (W[ids[t]] + P[pos(t)] + T[types[t]]),  pos(t) = t % S in the dense layout
and rowmap[t] % S in the packed one (a tail row, rowmap[t] < 0, is +0).  Backward: term[t] = keep[t] o scale dout[t] is added to row
ids[t] of dW, row pos(t) of dP and row types[t] of dT.

The mask.  csrc/rng.h is restated here in numpy uint32 arithmetic (mix32, row_hash, pair_bits, keep; drop_thr and keep_scale in float32 as
the header states them).  It is the first statement of the mask that does not come from a kernel: the GPU tests so far took it from
emdr2_dropout itself.  The effective probability is p quantised to 2^-16, so the EXACT scale of a float64 reference is the rational
65536 / (65536 - thr), not 1 / (1 - p): at p = 0.1 the two differ by 6.4e-6, a hundred fp32 roundoffs.

Bounds, derived, per element, against the sum of the MAGNITUDES of the terms (never |value|, never a tensor maximum):

    out (bf16)   C_BF16 scale (|W| + |P| + |T|) + ulp_bf16(ref) + TINY      kept elements; the sums are fp32, the store is bf16
    out (fp32)   C_F32        (|W| + |P| + |T|) + ulp_fp32(ref) + TINY      (the twin has no dropout)
                 a dropped element and every element of a tail row: bound 0, and the GPU tests check the bits (+0)
    dW, dP, dT   GRAD_WIDEN (n + 2) U32 sum_t |term| + TINY      n = the number of non-zero terms of the element (adding a zero is exact)
                 a recursive fp32 sum of n terms in ANY order (the atomics choose it; the position kernel's slice partials are one such
                 order) carries (n - 1) u sum |term|; one rounding more for the keep scale (fp32 of the rational), one for term = dout x
                 scale.  An element with sum |term| = 0 has bound 0 and must keep its previous contents BIT FOR BIT (`same_bits`).

Worst err / bound of the fp32 torch implementation of the same op on the CPU (`embedding_torch_f32`: index_add_ in float32, bf16 store
where the kernel stores bf16), over every ids x dout x types family below at p = 0, 1e-6, 0.1, 0.5, measured and asserted by
tests/test_embedding_ref_cpu.py.  The rule of tests/elementwise_ref.py applies: a bound whose reference ratio exceeds 0.5 is widened to
twice that ratio.

    quantity            worst ratio of the fp32 torch reference      constant
    out bf16 / fp32     0.25 / 0.02                                  C_BF16 / C_F32 (0.25 = half a bf16 ulp against 2^-7, plus one ulp)
    dW                  0.539 against (n + 2) U32 sum |term|         WIDENED: GRAD_WIDEN = 1.08 = 2 x 0.539 on the gradient formula
    dP / dT             0.454 / 0.207 against the same               (the same formula, so they carry GRAD_WIDEN too: 0.42 / 0.19)

The 0.539 is an element of ONE term at p = 0.1: the fp32 keep scale and the product dout x scale each round once, 1.6 u together against
3 u.  The derivation allows 2 u of 3 u there, so the rule, not the arithmetic, is what asks for the 8 %.

Input families (functions of the shape and a generator; every float operand is an fp32 tensor whose values are exact in bf16):

    ids     uniform; zipf (one id holds half of all tokens, a handful of ids appear exactly once); single (every token the same id);
            distinct (no id twice: dW rows are single terms, so dW = keep o scale dout row by row).
    dout    randn; row_scaled (token rows times 2^-20 .. 2^10 by id, the most frequent id at 2^10: a rare token's row is tiny next to
            the heavy one); sparse_rows (90 % of the rows zero, half of those all -0.0, which the zero-row skip must treat as zero);
            cancel (the tokens of one id come in +- pairs); coded (small integers, every column sum below 2^24: the fp32 sums are exact in
            any order -- compared with torch.equal, at p = 0 only).
    types   none; t1 .. t4 (n_types 1 .. 4, uniform); one_of_3 (every token type 1 of 3); skip_of_4 (type 2 of 4 never occurs: its dT row
            must stay untouched).

Out-of-range ids or types are not a family: they would read outside the tables.
"""
import numpy as np
import torch

from tests.elementwise_ref import C_BF16, C_F32, TINY, U32, Ref, _ulp, bf, old_metric, worst  # noqa: F401  (re-exported for the tests)

# ---- csrc/rng.h in numpy uint32 arithmetic ----------------------------------------------------------------------------------------------
_U = np.uint32
PAIR_MUL = _U(0x9e3779b1)


def _u32(x):
    return np.atleast_1d(np.asarray(x)).astype(np.uint32)


def mix32(x):
    """emdr2_mix32 (arrays wrap modulo 2^32 like the device's uint32_t)."""
    x = _u32(x).copy()
    x ^= x >> _U(16)
    x *= _U(0x7feb352d)
    x ^= x >> _U(15)
    x *= _U(0x846ca68b)
    x ^= x >> _U(16)
    return x


def row_hash(seed, rows):
    """emdr2_row_hash: rows are 64-bit row indices."""
    rows = np.atleast_1d(np.asarray(rows)).astype(np.uint64)
    lo, hi = (rows & np.uint64(0xffffffff)).astype(np.uint32), (rows >> np.uint64(32)).astype(np.uint32)
    s = _u32(int(seed) & 0xffffffff) * _U(0x9e3779b9) + _U(0x85ebca6b)
    return mix32(lo ^ mix32(hi + s))


def pair_bits(rowhash, col):
    """emdr2_pair_bits: 32 bits for the column pair (col & ~1, col | 1); rowhash and col broadcast."""
    x = ((_u32(col) >> _U(1)) * PAIR_MUL) ^ _u32(rowhash)
    x = x ^ (x >> _U(16))
    x = (x & _U(0xffffff)) * _U(0xa2d2e5)
    x = x ^ (x >> _U(15))
    return x


def keep(rowhash, col, thr):
    """emdr2_keep: the low half of the pair's bits for the even column, the high half for the odd one."""
    b = pair_bits(rowhash, col)
    half = np.where((_u32(col) & _U(1)) != 0, b >> _U(16), b & _U(0xffff))
    return half >= _U(thr)


def drop_thr(p):
    """emdr2_drop_thr in float32: (uint32_t)(p * 65536.f + 0.5f) (the product is exact, so a fused multiply-add gives the same)."""
    return int(np.float32(p) * np.float32(65536.0) + np.float32(0.5))


def keep_scale_f32(p):
    """emdr2_keep_scale in float32."""
    return float(np.float32(65536.0) / (np.float32(65536.0) - np.float32(drop_thr(p))))


def keep_scale_exact(p):
    """The rational 65536 / (65536 - thr) (as a float64) that a float64 reference scales survivors by."""
    return 65536.0 / (65536.0 - drop_thr(p))


def keep_bits(rows, cols, p, seed, device="cpu"):
    """bool [rows, cols]: True where (row, col) survives.  `rows`: a count (rows 0 .. rows - 1) or an array of row indices."""
    ridx = np.arange(rows, dtype=np.uint64) if np.isscalar(rows) else np.asarray(rows, dtype=np.uint64)
    if not p > 0.0:
        return torch.ones((len(ridx), cols), dtype=torch.bool, device=device)
    k = keep(row_hash(seed, ridx)[:, None], np.arange(cols, dtype=np.uint32)[None, :], drop_thr(p))
    return torch.from_numpy(k).to(device)


GRAD_WIDEN = 1.08                        # twice the fp32 torch reference's worst dW ratio, 0.539 (module docstring)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def _scatter(rows, idx, term):
    """-> (sum, count of non-zero terms, sum of magnitudes), each [rows, H] float64."""
    H = term.shape[1]
    z = lambda: torch.zeros((rows, H), dtype=torch.float64, device=term.device)
    return z().index_add_(0, idx, term), z().index_add_(0, idx, (term != 0).double()), z().index_add_(0, idx, term.abs())


def embedding_reference(ids, types, W, P, T, keep, scale, dout=None, S=None, cu=None, rowmap=None):
    """ids [b, S] (dense) or [rows] with `cu` [n + 1], `rowmap` [rows] and S (packed); types like ids or None; W [V, H], P [>= S, H],
    T [n_types, H] or None; keep bool [tokens, H] or None (everything kept); scale: the exact keep scale; dout [tokens, H] or None.
    -> Ref, float64: out [tokens, H]; dW, dP, dT with nW / aW, nP / aP, nT / aT (term counts and magnitude sums); kept [tokens, H] bool
    (False on tail rows); real [tokens] bool."""
    r = Ref()
    dev = W.device
    if rowmap is None:
        S = ids.shape[1]
        idf = ids.reshape(-1)
        pos = torch.arange(idf.numel(), device=dev) % S
        real = torch.ones_like(idf, dtype=torch.bool)
    else:
        idf = ids.reshape(-1)
        real = rowmap >= 0
        pos = torch.where(real, rowmap.long() % S, torch.zeros_like(idf))
        if cu is not None:                                               # the two statements of the layout must agree
            lens = (cu[1:] - cu[:-1]).long()
            assert int(cu[-1]) == int(real.sum()) and bool((lens >= 1).all()) and bool((lens <= S).all())
            start = torch.repeat_interleave(cu[:-1].long(), lens)
            assert torch.equal(pos[real], torch.arange(int(cu[-1]), device=dev) - start)
    tyf = None if types is None or T is None else types.reshape(-1)
    Wd, Pd = W.double(), P.double()
    mag = Wd[idf].abs() + Pd[pos].abs()
    val = Wd[idf] + Pd[pos]
    if tyf is not None:
        mag, val = mag + T.double()[tyf].abs(), val + T.double()[tyf]
    kept = real[:, None].expand_as(val) if keep is None else keep & real[:, None]
    r.scale = float(scale)
    r.out = torch.where(kept, val * r.scale, torch.zeros_like(val))
    r.mag = torch.where(kept, mag * r.scale, torch.zeros_like(mag))
    r.kept, r.real, r.pos, r.ids, r.types = kept, real, pos, idf, tyf
    r.dout = None
    if dout is not None:
        r.dout = dout.double()
        r.term = torch.where(kept, r.dout * r.scale, torch.zeros_like(r.dout))
        r.dW, r.nW, r.aW = _scatter(W.shape[0], idf, r.term)
        r.dP, r.nP, r.aP = _scatter(P.shape[0], pos, r.term)
        if tyf is not None:
            r.dT, r.nT, r.aT = _scatter(T.shape[0], tyf, r.term)
    return r


def embedding_bounds(r, c=C_BF16, mant_bits=7):
    """out (+ dW, dP, dT).  c / mant_bits describe the format `out` is stored in; the gradients are fp32 sums either way."""
    B = {"out": torch.where(r.kept, c * r.mag + _ulp(r.out, mant_bits) + TINY, torch.zeros_like(r.out))}
    if r.dout is not None:
        grad = lambda n, a: torch.where(a > 0, GRAD_WIDEN * (n + 2.0) * U32 * a + TINY, torch.zeros_like(a))
        B["dW"], B["dP"] = grad(r.nW, r.aW), grad(r.nP, r.aP)
        if r.types is not None:
            B["dT"] = grad(r.nT, r.aT)
    return B


def same_bits(a, b):
    """Bit-for-bit equality of two tensors of one dtype (-0.0 != +0.0, NaN == the same NaN)."""
    ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.contiguous().view(ints) == b.contiguous().view(ints)


def untouched_ok(after, before, mag):
    """True when every element whose terms sum to zero in magnitude still holds its previous contents bit for bit."""
    return bool((same_bits(after, before) | (mag > 0)).all())


def worst_grads(got, before, r, B):
    """{name: (ratio, index)} of after - before against the reference sums, an element whose bits changed without a term counting as
    infinitely wrong.  got / before: dicts of fp32 tensors dW, dP (+ dT)."""
    res = {}
    for n in B:
        if n == "out":
            continue
        ref, mag = getattr(r, n), getattr(r, "a" + n[1])
        delta = got[n].double() - before[n].double()
        # the pre-filled value is one more term of the same recursive sum: (n + 1 + 2) u (|before| + sum |term|)
        pre = before[n].double().abs()
        cnt = getattr(r, "n" + n[1])
        bound = torch.where(mag > 0, B[n] + torch.where(pre > 0, (cnt + 3.0) * U32 * pre + U32 * mag, torch.zeros_like(pre)), B[n])
        ratio, idx = worst(delta, ref, bound)
        if not untouched_ok(got[n], before[n], mag):
            ratio = float("inf")
        res[n] = (ratio, idx)
    return res


def embedding_torch_f32(r, W, P, T, dout, scale_f32, store_bf16=True):
    """The fp32 torch implementation of the same op on the layout of Ref r: ((W + P) + T) x scale, index_add_ in float32."""
    rnd = bf if store_bf16 else (lambda t: t)
    v = W.float()[r.ids] + P.float()[r.pos]
    if r.types is not None:
        v = v + T.float()[r.types]
    s = torch.tensor(scale_f32, dtype=torch.float32, device=W.device)
    got = {"out": rnd(torch.where(r.kept, v * s, torch.zeros_like(v)))}
    if dout is not None:
        g = torch.where(r.kept, dout.float() * s, torch.zeros_like(v))
        got["dW"] = torch.zeros(W.shape, dtype=torch.float32, device=W.device).index_add_(0, r.ids, g)
        got["dP"] = torch.zeros(P.shape, dtype=torch.float32, device=W.device).index_add_(0, r.pos, g)
        if r.types is not None:
            got["dT"] = torch.zeros(T.shape, dtype=torch.float32, device=W.device).index_add_(0, r.types, g)
    return got


# ---- input families -------------------------------------------------------------------------------------------------------------------
IDS_FAMILIES = ("uniform", "zipf", "single", "distinct")
DOUT_FAMILIES = ("randn", "row_scaled", "sparse_rows", "cancel")
EXACT_DOUT_FAMILIES = ("coded",)
TYPES_FAMILIES = ("none", "t1", "t2", "t3", "t4", "one_of_3", "skip_of_4")
HEAVY_ID = 3


def vocab_for(fam, n):
    """The smallest table the family needs for n tokens (distinct: a row per token)."""
    return max(n + 2, 16) if fam == "distinct" else 64


def ids_inputs(fam, n, V, gen, device="cpu", lo=0):
    """n token ids in [lo, V) (lo = 1: a packed layout's real tokens, which are never 0)."""
    ri = lambda a, b, *s: torch.randint(a, b, s, generator=gen, device=device)
    if fam == "uniform":
        return ri(lo, V, n)
    if fam == "single":
        return torch.full((n,), 7 % V, dtype=torch.int64, device=device)
    if fam == "distinct":
        if V - lo < n:
            raise ValueError("distinct ids need a table row per token")
        return lo + torch.randperm(V - lo, generator=gen, device=device)[:n]
    if fam == "zipf":
        once = min(5, n // 4)                                            # ids V - 1, V - 2, ...: exactly once each
        ids = ri(HEAVY_ID + 1, V - 5, n)
        order = torch.randperm(n, generator=gen, device=device)
        ids[order[:(n + 1) // 2]] = HEAVY_ID
        if once:
            ids[order[n - once:]] = V - 1 - torch.arange(once, device=device)
        return ids
    raise ValueError(fam)


def types_inputs(fam, n, gen, device="cpu"):
    """-> (types [n] or None, n_types)."""
    if fam == "none":
        return None, 0
    if fam == "one_of_3":
        return torch.ones(n, dtype=torch.int64, device=device), 3
    if fam == "skip_of_4":
        t = torch.randint(0, 3, (n,), generator=gen, device=device)
        return torch.where(t == 2, torch.full_like(t, 3), t), 4
    k = int(fam[1:])
    return torch.randint(0, k, (n,), generator=gen, device=device), k


def dout_inputs(fam, ids, H, gen, device="cpu"):
    """[n, H] fp32 holding bf16 values, a function of the flat ids (the families are about tokens that share a table row)."""
    n = ids.numel()
    rn = lambda *s: torch.randn(s, generator=gen, device=device)
    if fam == "randn":
        return bf(rn(n, H))
    if fam == "row_scaled":
        e = ((ids * 7) % 31 - 20).double()
        e = torch.where(ids == torch.mode(ids.cpu()).values.to(device), torch.full_like(e, 10.0), e)
        return bf(rn(n, H) * torch.exp2(e).float()[:, None])
    if fam == "sparse_rows":
        d = bf(rn(n, H))
        u = torch.rand(n, generator=gen, device=device)
        d[u < 0.9] = 0.0
        d[u < 0.45] = -0.0
        return d
    if fam == "cancel":
        d = bf(rn(n, H))
        order = torch.argsort(ids, stable=True)
        sid = ids[order]
        first = torch.ones(n, dtype=torch.bool, device=device)
        first[1:] = sid[1:] != sid[:-1]
        start = torch.cummax(torch.where(first, torch.arange(n, device=device), torch.zeros(n, dtype=torch.int64, device=device)), 0).values
        odd = (torch.arange(n, device=device) - start) % 2 == 1          # the 2nd, 4th, ... token of an id: minus the one before
        src = order[torch.arange(n, device=device) - 1]
        d[order[odd]] = -d[src[odd]]
        return d
    if fam == "coded":                                                   # integers in [-8, 8]: |column sum| <= 8 n < 2^24 for n < 2^21
        if n >= 1 << 21:
            raise ValueError("coded: too many tokens for exact fp32 sums")
        t, i = torch.arange(n, device=device)[:, None], torch.arange(H, device=device)[None, :]
        return ((t * 31 + i * 7 + ids[:, None] * 3) % 17 - 8).float()
    raise ValueError(fam)


def tables(V, rows_p, n_types, H, gen, device="cpu"):
    """W [V, H], P [rows_p, H], T [n_types, H] or None: fp32 holding bf16 values; row 0 of W (the padding token's) 4,096 times larger."""
    rn = lambda *s: torch.randn(s, generator=gen, device=device)
    W = rn(V, H)
    W[0] *= 4096.0
    return bf(W), bf(rn(rows_p, H)), (bf(rn(n_types, H)) if n_types else None)


def sentinel(shape, device="cpu"):
    """A pre-fill for dW / dP / dT: values that differ from element to element (multiples of 2^-6 around +-300, exact in fp32), every
    seventh element -0.0 and every eleventh +0.0: adding a +0.0 changes the bits of a -0.0 and of nothing else."""
    n = 1
    for d in shape:
        n *= d
    i = torch.arange(n, device=device)
    v = ((i * 37) % 4099).float() * 0.015625 + 300.0
    v = torch.where(i % 3 == 0, -v, v)
    v = torch.where(i % 7 == 0, torch.full_like(v, -0.0), v)
    return torch.where(i % 11 == 0, torch.zeros_like(v), v).reshape(shape)
