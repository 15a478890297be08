"""CPU: the C-ABI library loads and exports every symbol include/emdr2_mips.h declares; argument
validation works without touching a GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from emdr2_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        g.build()
    return _native.lib()


def _declared():
    names = set()
    for h in sorted(os.listdir(os.path.join(ROOT, "include"))):
        text = open(os.path.join(ROOT, "include", h)).read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        names |= set(re.findall(r"\bint\s+(emdr2_\w+)\s*\(", text))
    return sorted(names)


def test_every_declared_symbol_is_exported_and_bound(lib):
    from emdr2_amd import _native
    names = _declared()
    assert len(names) >= 12
    for n in names:
        assert hasattr(lib, n), "library does not export %s" % n
        assert n in _native.SIGNATURES, "ctypes binding missing for %s" % n
    assert sorted(_native.SIGNATURES) == names, "binding table and header drifted"


def test_abi_version(lib):
    assert lib.emdr2_abi_version() == 4          # r06: the validation-only fp32 compute path (include/emdr2_ops_f32.h); r05: packed records


def test_layout_bytes_and_argument_validation(lib):
    n = ctypes.c_size_t()
    assert lib.emdr2_mips_layout_bytes(21015324, 768, ctypes.byref(n)) == 0
    assert n.value == ((21015324 + 511) // 512 * 512) * 768 * 2
    assert lib.emdr2_mips_layout_bytes(10, 100, ctypes.byref(n)) == -1        # dim % 32 != 0
    assert lib.emdr2_mips_layout_bytes(10, 32, ctypes.byref(n)) == -1         # dim < 64
    assert lib.emdr2_mips_workspace_bytes(512, 768, 50, ctypes.byref(n)) == 0 and n.value > 512 * 16384 * 8
    assert lib.emdr2_mips_workspace_bytes(512, 768, 121, ctypes.byref(n)) == -1
    # null pointers are rejected before any launch
    assert lib.emdr2_mips_search(None, 10, 768, 0, None, None, 1, 5, None, None, None, None, None, None, 0, None) == -1
    assert lib.emdr2_mips_merge(None, None, None, 2, 4, 5, None, None, None, None) == -1


def test_missing_library_fails_loudly(monkeypatch):
    from emdr2_amd import _native
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setattr(_native, "LIB_PATH", "/nonexistent/libemdr2_hip.so")
    with pytest.raises(_native.NativeError):
        _native.lib()


def test_index_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from emdr2_amd import _native
    from emdr2_amd.data.emdr2_index import HipIndexShard
    with pytest.raises(_native.NativeError):
        HipIndexShard(768, 100, 0)


def test_ops_entry_points_validate_arguments_without_a_gpu(lib):
    """Bad shapes / null pointers come back as status codes before any launch (no exceptions across the ABI)."""
    n = ctypes.c_size_t()
    assert lib.emdr2_mips_exact_workspace_bytes_f32(1000, 4, ctypes.byref(n)) == 0 and n.value >= 8 * 1000 * 4
    assert lib.emdr2_mips_search_f32(None, 10, 768, 0, None, None, 1, 5, None, None, None, None, None, None, 0, None) == -1
    assert lib.emdr2_mips_merge_f32(None, None, None, 2, 4, 5, None, None, None, None) == -1
    one = ctypes.c_void_p(4096)                                          # a non-null, 16-byte aligned fake pointer: shapes are checked first
    # GEMM: K must be a multiple of 32, split-K only with fp32 output and no epilogue, dropout only unbatched
    assert lib.emdr2_gemm_nt_bf16(one, 64, one, 64, one, 64, 16, 16, 40, 1, 0, 0, 0, 1, 0, 0, 0, 1.0, None, 0, None, None, 0, 0, 1, 0.0, 0, None) == -1
    assert lib.emdr2_gemm_nt_bf16(one, 64, one, 64, one, 64, 16, 16, 64, 1, 0, 0, 0, 1, 0, 0, 0, 1.0, None, 0, None, None, 0, 0, 2, 0.0, 0, None) == -1
    assert lib.emdr2_gemm_nt_bf16(one, 64, one, 64, one, 64, 16, 16, 64, 2, 0, 0, 0, 1, 0, 0, 0, 1.0, None, 0, None, None, 0, 0, 1, 0.1, 7, None) == -1
    assert lib.emdr2_gemm_nt_bf16(one, 64, one, 64, one, 64, 16, 16, 64, 1, 0, 0, 0, 1, 0, 0, 0, 1.0, None, 0, None, None, 3, 0, 1, 0.0, 0, None) == -1      # residual_mode is 0, 1 or 2
    assert lib.emdr2_gemm_nt_bf16(one, 64, one, 64, one, 64, 16, 16, 64, 1, 0, 0, 0, 1, 0, 0, 0, 1.0, None, 2, None, None, 0, 0, 1, 0.0, 0, None) == -1      # gelu = 2 needs pre_act
    assert lib.emdr2_gemm_tn_bf16(one, 64, one, 64, one, 64, 64, 64, 48, 1, None, None) == -1      # R % 32
    assert lib.emdr2_gemm_tn_bf16(None, 64, one, 64, one, 64, 64, 64, 64, 1, None, None) == -1
    # attention: head dim 64 and sk % 32 == 0 only (-4 = unsupported shape, the caller falls back to the composed path)
    args_f = (one, 64, 64, 64, one, 64, 64, 64, one, 64, 64, 64, one, one, one, 1, 1, 32)
    assert lib.emdr2_attention_fwd(*args_f, 72, 64, 0, 0.125, 0.0, 0, None, None, None) == -4
    assert lib.emdr2_attention_fwd(*args_f, 128, 32, 0, 0.125, 0.0, 0, None, None, None) == -4
    assert lib.emdr2_attention_fwd(*args_f, 128, 64, 0, 0.125, 1.5, 0, None, None, None) == -1
    assert lib.emdr2_dropout(one, one, 64, 12, 0.1, 1, None) == -1          # cols % 8
    assert lib.emdr2_layernorm_fwd(one, one, one, one, one, one, 4, 12, 1e-5, None) == -1


def test_r05_entry_points_validate_their_arguments(lib):
    """The packed-record exchange and the split-key attention entries (ABI 3): bad pointers are refused without touching a GPU, and the
    split-key plan -- a pure function of the query / key extents, never of the batch -- says what include/emdr2_ops.h says."""
    assert lib.emdr2_mips_search_records(None, 10, 64, 0, None, None, 1, 1, None, 0, None, None, None, 0, None) == -1
    assert lib.emdr2_mips_merge_records(None, 2, 4, 5, 0, None, None, None, None) == -1
    assert lib.emdr2_mips_pack_records(None, None, None, None, 0, 5, 0, None, None) == -1
    ks, fb, bb = ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()

    def plan(batch, heads, sq, sk):
        assert lib.emdr2_attention_splitkv_plan(batch, heads, sq, sk, ctypes.byref(ks), ctypes.byref(fb), ctypes.byref(bb)) == 0
        return ks.value, fb.value, bb.value
    assert plan(16, 12, 32, 25600) == (13, 13 * 16 * 12 * 32 * 66 * 4, 13 * 16 * 12 * 32 * 64 * 4)       # 400 key blocks in ranges of 32
    assert plan(64, 12, 32, 25600)[0] == plan(1, 12, 32, 25600)[0] == 13                               # the batch does not enter
    assert plan(16, 12, 32, 4095) == (1, 0, 0) and plan(16, 12, 32, 4096)[0] == 2                       # short key sets never split
    assert plan(16, 12, 129, 25600) == (1, 0, 0) and plan(16, 12, 128, 65536)[0] == 32                 # one query block only
    assert lib.emdr2_attention_splitkv_plan(0, 12, 32, 25600, ctypes.byref(ks), ctypes.byref(fb), ctypes.byref(bb)) == -1


_ONE = ctypes.c_void_p(4096)               # a non-null, 16-byte aligned fake pointer: every row below returns before any launch


def _attn_call(lib, entry, **kw):
    """One attention entry with batch = heads = 1, every stride 64, head dim 64, sq 32, every pointer the fake aligned one, unless `kw` says otherwise."""
    a = dict(batch=1, heads=1, sq=32, sk=64, head_dim=64, causal=0, scale=0.125, drop_p=0.0, seed=0, cu_q=None, cu_k=None, total_q=0, pairs=0,
             ksplit=1, ws=None, ws_bytes=0, q=_ONE, dq=_ONE, q_ss=64, dq_ss=64)
    assert set(kw) <= set(a), kw
    a.update(kw)
    qkv = (a["q"], 64, a["q_ss"], 64, _ONE, 64, 64, 64, _ONE, 64, 64, 64)
    bwd = entry.endswith("bwd") or "bwd_" in entry
    ptrs = (_ONE, _ONE, a["dq"], 64, a["dq_ss"], _ONE, _ONE, 64, 64, _ONE, _ONE) if bwd else (_ONE, _ONE, _ONE)     # o [dout dq .. dkv_ss] ids_q ids_k
    stats = (_ONE, _ONE, _ONE) if bwd else ()                                                                        # m l dstat (the forward's m, l: the tail)
    shape = (a["batch"], a["heads"], a["sq"], a["sk"], a["head_dim"], a["causal"], a["scale"], a["drop_p"], a["seed"])
    tail = () if bwd else (_ONE, _ONE)
    if "splitkv" in entry:
        args = qkv + ptrs + (a["cu_k"], a["pairs"]) + stats + shape + tail + (a["ksplit"], a["ws"], a["ws_bytes"], None)
    elif "varlen" in entry:
        args = qkv + ptrs + (a["cu_q"], a["cu_k"], a["total_q"], a["pairs"]) + stats + shape + tail + (None,)
    else:
        args = qkv + ptrs + stats + shape + tail + (None,)
    return getattr(lib, entry)(*args)


# (entry, arguments, code): the codes are what the library returned BEFORE the launchers were rewritten on shared validators; the order of the
# checks decides which code a doubly-wrong call gets (null pointers -1, ksplit -1, shape / strides -4, packed row count -1, alignment and
# drop_p -1, workspace size -2), and the forward splits only at >= 4,096 keys while the backward accepts any sk whose ranges match.
_ATTN_CODES = [
    ("emdr2_attention_fwd_splitkv", dict(sk=2048, ksplit=2, ws=_ONE, ws_bytes=1 << 30), -1),       # the forward does not split below 4,096 keys
    ("emdr2_attention_fwd_splitkv", dict(sk=4096, ksplit=2, ws=None), -1),
    ("emdr2_attention_fwd_splitkv", dict(sk=4096, ksplit=2, ws=_ONE, ws_bytes=0), -2),
    ("emdr2_attention_fwd_splitkv", dict(sq=129, sk=4096, ksplit=2, ws=_ONE, ws_bytes=1 << 30), -1),
    ("emdr2_attention_fwd_splitkv", dict(ksplit=1, ws=None, head_dim=32), -4),
    ("emdr2_attention_bwd_splitkv", dict(sk=2112, ksplit=2, ws=_ONE, ws_bytes=0), -2),             # the backward has no 4,096 floor
    ("emdr2_attention_fwd_splitkv", dict(sk=2112, ksplit=2, ws=_ONE, ws_bytes=0), -1),
    ("emdr2_attention_bwd_splitkv", dict(sq=129, sk=4096, ksplit=2, ws=_ONE, ws_bytes=1 << 30), -1),
    ("emdr2_attention_varlen_fwd", dict(), -1),                                                    # neither side packed
    ("emdr2_attention_varlen_bwd", dict(), -1),
    ("emdr2_attention_varlen_fwd", dict(cu_q=_ONE, total_q=0), -1),
    ("emdr2_attention_varlen_fwd", dict(cu_q=_ONE, total_q=0, head_dim=32), -4),                   # the shape check comes first
    ("emdr2_attention_bwd", dict(dq_ss=60), -4),
    ("emdr2_attention_bwd", dict(drop_p=1.0), -1),
    # the same orderings seen from the other launcher, and each kind of check once per direction
    ("emdr2_attention_varlen_fwd", dict(cu_q=_ONE, total_q=0, q_ss=60), -4),                       # forward: strides with the shape, before the row count
    ("emdr2_attention_varlen_bwd", dict(cu_q=_ONE, total_q=0, q_ss=60), -1),                       # backward: the row count before the strides
    ("emdr2_attention_varlen_bwd", dict(cu_q=_ONE, total_q=0, head_dim=32), -4),
    ("emdr2_attention_fwd", dict(q_ss=60), -4),
    ("emdr2_attention_fwd", dict(q=ctypes.c_void_p(4104)), -1),
    ("emdr2_attention_fwd", dict(q=ctypes.c_void_p(4104), sk=72), -4),                             # dense keys: whole 32-key steps, before alignment
    ("emdr2_attention_fwd", dict(q=None, head_dim=32), -1),                                        # null pointers before everything
    ("emdr2_attention_fwd", dict(sk=65568), -4),
    ("emdr2_attention_bwd", dict(sk=72), -4),
    ("emdr2_attention_bwd", dict(dq=ctypes.c_void_p(4100)), -1),
    ("emdr2_attention_bwd", dict(dq=None, sk=72), -1),
    ("emdr2_attention_bwd", dict(heads=1 << 16), -4),                                              # 32-bit lane offsets of the dk / dv staging
    ("emdr2_attention_bwd_splitkv", dict(sk=4096, ksplit=3, ws=_ONE, ws_bytes=1 << 30), -1),       # not the number of ranges of 4,096 keys
    ("emdr2_attention_bwd_splitkv", dict(sk=4096, ksplit=2, ws=ctypes.c_void_p(4104), ws_bytes=1 << 30), -1),
    ("emdr2_attention_bwd_splitkv", dict(sk=4096, ksplit=2, ws=_ONE, ws_bytes=1 << 30, head_dim=32), -4),
    ("emdr2_attention_fwd_splitkv", dict(sk=4096, ksplit=65, ws=_ONE, ws_bytes=1 << 30), -1),
    ("emdr2_attention_fwd_splitkv", dict(sk=4096, ksplit=0), -1),
    ("emdr2_attention_varlen_fwd", dict(cu_k=_ONE, sk=72, drop_p=-0.5), -1),                       # packed keys take any length
]


@pytest.mark.parametrize("row", range(len(_ATTN_CODES)))
def test_attention_entry_points_keep_their_return_codes(lib, row):
    entry, kw, code = _ATTN_CODES[row]
    assert _attn_call(lib, entry, **kw) == code, (entry, kw)


def test_fp32_validation_entry_points_validate_their_arguments(lib):
    """include/emdr2_ops_f32.h (ABI 4): null pointers / empty shapes are refused before any launch."""
    one = ctypes.c_void_p(4096)
    assert lib.emdr2_f32_gemm(None, 1, 1, 0, 0, one, 1, 1, 0, 0, one, 1, 1, 0, 0, 4, 4, 4, 1, 1, 1.0, None, None, 0, None) == -1
    assert lib.emdr2_f32_gemm(one, 1, 1, 0, 0, one, 1, 1, 0, 0, one, 1, 1, 0, 0, 4, 4, 0, 1, 1, 1.0, None, None, 0, None) == -1
    assert lib.emdr2_f32_layernorm_fwd(one, one, one, one, one, None, 4, 16, 1e-5, None) == -1
    assert lib.emdr2_f32_layernorm_bwd(one, one, one, one, one, None, one, one, None, 4, 16, None) == -1
    assert lib.emdr2_f32_softmax_mask_fwd(one, one, None, 1, 1, 4, 4, 0, None) == -1
    assert lib.emdr2_f32_softmax_mask_bwd(one, None, one, one, 1, 1, 4, 4, 0, None) == -1
    assert lib.emdr2_f32_gelu_fwd(one, None, 8, None) == -1 and lib.emdr2_f32_gelu_bwd(one, one, one, 0, None) == -1
    assert lib.emdr2_f32_embedding_fwd(one, None, one, one, one, one, 4, 4, 16, None) == -1      # a token-type table without token types
    assert lib.emdr2_f32_embedding_bwd(one, None, one, one, None, None, 4, 4, 16, None) == -1
    assert lib.emdr2_f32_lse_gather_fwd(one, one, one, None, 4, 16, None) == -1
    assert lib.emdr2_f32_lse_gather_bwd(one, one, one, one, None, 4, 16, None) == -1
    assert lib.emdr2_f32_retriever_prior_fwd(one, one, one, one, 2, 2000, 16, 1.0, None) == -1    # K <= 1024
    assert lib.emdr2_f32_retriever_prior_bwd(one, one, one, one, one, None, 2, 4, 16, 1.0, None) == -1


def test_assemble_evidence_validates_its_arguments(lib):
    """include/emdr2_assembly.h: null pointers, shapes the kernel cannot lay out and a null table inside the arena struct are refused (-1)
    before any launch."""
    from emdr2_amd import _native
    one = ctypes.c_void_p(4096)
    arena = _native.EvidenceArenaStruct()
    tables = [f[0] for f in arena._fields_ if f[0] != "n_docs"]
    assert len(tables) == 8
    for t in tables:
        setattr(arena, t, 4096)
    arena.n_docs = 10

    def call(arena_p=ctypes.byref(arena), ptrs=(one,) * 9, n_b=2, k_retrieved=4, topk=3, q_stride=8, s_ret=12, s=24):
        ids, uid, q, ql, ctx, typ, ext, one_, kept = ptrs
        return lib.emdr2_assemble_evidence(arena_p, ids, n_b, k_retrieved, topk, uid, q, q_stride, ql, s_ret, s, 2, 3, 0, ctx, typ, ext, one_, kept, None)
    assert call(arena_p=None) == -1
    for i in range(9):                                                   # topk_ids, query_uid, query_t5, query_len and the five outputs
        assert call(ptrs=tuple(None if j == i else one for j in range(9))) == -1, i
    assert call(k_retrieved=2) == -1                                     # k_retrieved < topk
    assert call(topk=0, k_retrieved=0) == -1
    assert call(s=1) == -1 and call(s_ret=1) == -1                       # a row holds at least one token and the closing [SEP]
    assert call(q_stride=0) == -1
    assert call(n_b=0) == -1 and call(n_b=-3) == -1
    for t in tables:                                                     # a null table inside the arena struct
        setattr(arena, t, None)
        assert call() == -1, t
        setattr(arena, t, 4096)


def test_vector_cast_entry_points_reject_odd_lengths_and_misaligned_pointers(lib):
    """The four-elements-per-thread kernels (gradient exchange casts, flat Adam) take n % 4 == 0, 16-byte aligned fp32 and 8-byte aligned
    bf16 pointers: anything else is refused (-1) before a launch; LayerNorm backward + mask takes H = 768 only (-4)."""
    al, off4, off8 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4), ctypes.c_void_p(4096 + 8)
    for n in (1, 6, 1027):
        assert lib.emdr2_scale_cast_f32_to_bf16(al, al, n, 1.0, None) == -1
        assert lib.emdr2_widen_bf16_to_f32(al, al, n, None) == -1
        assert lib.emdr2_adam_step_flat(al, al, al, al, al, n, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, 0.0, None) == -1
    assert lib.emdr2_scale_cast_f32_to_bf16(off8, al, 1028, 1.0, None) == -1       # fp32 source: 16 bytes
    assert lib.emdr2_scale_cast_f32_to_bf16(al, off4, 1028, 1.0, None) == -1       # bf16 destination: 8 bytes
    assert lib.emdr2_widen_bf16_to_f32(al, off8, 1028, None) == -1
    assert lib.emdr2_widen_bf16_to_f32(off4, al, 1028, None) == -1
    for bad in range(4):
        ptrs = [off8 if i == bad else al for i in range(4)]
        assert lib.emdr2_adam_step_flat(ptrs[0], ptrs[1], ptrs[2], ptrs[3], al, 1028, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, 0.0, None) == -1
    assert lib.emdr2_adam_step_flat(al, al, al, al, off4, 1028, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, 0.0, None) == -1
    assert lib.emdr2_adam_step_flat(al, al, al, al, al, 1028, 6, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, 0.0, None) == -1      # split % 4
    assert lib.emdr2_adam_step_flat(al, al, al, al, al, 1028, 1032, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, 0.0, None) == -1   # split > n
    assert lib.emdr2_adam_step_flat(al, al, al, al, al, 1028, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, None, 0.0, None) == -1      # step < 1
    assert lib.emdr2_layernorm_bwd_mask(al, al, al, al, al, None, al, al, al, 4, 264, al, 0.1, 1, None) == -4
    assert lib.emdr2_retriever_prior_fwd(al, al, al, al, 2, 1025, 64, 1.0, None) == -4
