"""No GPU: the host side of the ordered-sum gradient entries (include/emdr2_ops.h, "Ordered sums").  The float64 restatement of
tests/ordered_grads_ref.py against per-element loops, the rules of --deterministic-gradients, the ctypes signatures, the new kernels in the
built library (no scratch, read the way tests/test_isa_budget.py reads it) and the argument checks that need no device."""
import ctypes
import os
import sys

import numpy as np
import pytest

from tests import ordered_grads_ref as R
from tests.test_context_from_index_cpu import BASE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources as kr  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from emdr2_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        g.build()
    return _native.lib()


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
def test_bf16_rounding_and_bits():
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.140625, 2.0 ** -20], dtype=np.float32)
    assert R.to_bf16(a).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, -3.140625, 2.0 ** -20]        # ties to even, both ways
    assert R.bf16_bits(np.array([1.0, -2.0], dtype=np.float32)).view(np.uint16).tolist() == [0x3f80, 0xc000]
    s = R.spread((64, 64), np.random.default_rng(0))
    assert np.array_equal(R.to_bf16(s), s) and np.abs(s).max() > 2.0 ** 15 and np.abs(s[s != 0]).min() < 2.0 ** -15


def test_gamma_and_bound():
    assert R.gamma(1) == pytest.approx(2.0 ** -24, rel=1e-6) and R.gamma(4096) > 4096 * 2.0 ** -24
    assert R.sum_bound(1.0, 10) == pytest.approx(13 * 2.0 ** -24, rel=1e-5)
    assert R.sum_bound(1.0, 10, prefill_abs=3.0, e_term=R.gamma(1)) == pytest.approx(4 * (13 + 1) * 2.0 ** -24, rel=1e-5)


def test_tn_reference_against_the_loop():
    rng = np.random.default_rng(1)
    A, B = R.spread((96, 16), rng, -4, 4), R.spread((96, 24), rng, -4, 4)
    dW, S, cs, Scs = R.tn_reference(A, B)
    for i, j in ((0, 0), (15, 23), (7, 11)):
        s, m = R.tn_reference_loop(A, B, i, j)
        assert dW[i, j] == pytest.approx(s, rel=1e-12, abs=1e-12 * m) and S[i, j] == pytest.approx(m, rel=1e-12)
    assert cs[3] == pytest.approx(float(A[:, 3].astype(np.float64).sum()), rel=1e-12, abs=1e-9) and Scs[3] == pytest.approx(np.abs(A[:, 3]).sum(), rel=1e-6)


def test_ln_reference_against_the_loop():
    rng = np.random.default_rng(2)
    dy, x = R.spread((33, 8), rng, -3, 3), R.to_bf16(rng.standard_normal((33, 8)))
    mean, rstd = x.mean(1).astype(np.float32), (1.0 / np.sqrt(x.var(1) + 1e-5)).astype(np.float32)
    dg, Sg, db, Sb = R.ln_reference(dy, x, mean, rstd)
    for c in (0, 7):
        sg, mg, sb, mb = R.ln_reference_loop(dy, x, mean, rstd, c)
        assert dg[c] == pytest.approx(sg, rel=1e-12, abs=1e-12 * mg) and Sg[c] == pytest.approx(mg, rel=1e-12)
        assert db[c] == pytest.approx(sb, rel=1e-12, abs=1e-12 * mb) and Sb[c] == pytest.approx(mb, rel=1e-12)


def test_embedding_reference_against_the_loop():
    rng = np.random.default_rng(3)
    n, H, V, S = 48, 8, 7, 8
    ids, types = rng.integers(0, 5, n), rng.integers(0, 3, n)
    pos = np.tile(np.arange(S), n // S)
    pos[-3:] = -1                                                    # tail rows: no position, no type
    dout, keep = R.spread((n, H), rng, -3, 3), rng.random((n, H)) > 0.2
    out = R.embedding_reference(ids, types, dout, keep, 1.25, pos, V, S + 2, 3)
    for v, c in ((0, 0), (4, 7), (6, 3)):
        s, m, cnt = R.embedding_reference_loop(ids, dout, keep, 1.25, v, c)
        assert out["dW"][0][v, c] == pytest.approx(s, rel=1e-12, abs=1e-12) and out["dW"][1][v, c] == pytest.approx(m, rel=1e-12) and out["dW"][2][v] == cnt
    assert out["dW"][2][5] == 0 and out["dW"][2][6] == 0 and not out["dW"][0][5:].any()
    assert out["dP"][2][S:].sum() == 0 and out["dP"][2].sum() == n - 3 and out["dT"][2].sum() == n - 3
    g = np.where(keep, dout.astype(np.float64) * 1.25, 0.0)
    assert out["dP"][0][2] == pytest.approx(g[(pos == 2)].sum(0), rel=1e-12, abs=1e-12)
    assert out["dT"][0][1] == pytest.approx(g[(types == 1) & (pos >= 0)].sum(0), rel=1e-12, abs=1e-12)


# ---- the flag ----------------------------------------------------------------------------------------------------------------------------------
def test_flag_rules():
    from emdr2_amd import arguments
    assert arguments.parse_args(BASE).deterministic_gradients is False
    assert arguments.parse_args(BASE + ["--deterministic-gradients"]).deterministic_gradients is True
    assert "--deterministic-gradients" in arguments.get_parser().format_help()
    with pytest.raises(ValueError, match="fp32-validation"):
        arguments.parse_args(BASE + ["--deterministic-gradients", "--fp32-validation"])


def test_switch_is_off_by_default_and_holds_no_workspace():
    from emdr2_amd.model import kernels as K
    assert K.ORDERED.enabled is False and K.ORDERED._ws == {} and K.ORDERED.calls == 0


# ---- the library -------------------------------------------------------------------------------------------------------------------------------
NEW = ("emdr2_gemm_tn_ordered_ws_bytes", "emdr2_gemm_tn_bf16_ordered", "emdr2_layernorm_bwd_ordered_ws_bytes", "emdr2_layernorm_bwd_ordered",
       "emdr2_embedding_bwd_ordered_ws_bytes", "emdr2_embedding_bwd_ordered")


def test_signatures_are_present(lib):
    from emdr2_amd import _native
    hdr = open(os.path.join(ROOT, "include", "emdr2_ops.h")).read()
    for name in NEW:
        assert name in _native.SIGNATURES and name + "(" in hdr
        assert getattr(lib, name).argtypes == _native.SIGNATURES[name][1]


@pytest.mark.skipif(not (os.path.exists(kr.DEFAULT_LIB) and os.path.exists(os.path.join(kr.LLVM, "llvm-readelf"))), reason="needs the built library and llvm-readelf")
def test_library_holds_the_ordered_kernels_without_scratch():
    table = kr.kernels()
    for sub, count in (("gemm8t_kernelILb1E", 1), ("gemm_tn_kernelILb1E", 1), ("layernorm_bwd_kernelILb1E", 1), ("layernorm_bwd768_kernelILb0ELb1E", 1),
                       ("layernorm_bwd768_kernelILb1ELb1E", 1), ("embedding_bwd_pos_kernelILb1E", 1), ("embedding_bwd_words_ordered_kernel", 2),
                       ("embedding_bwd_words_finish_kernel", 2), ("ordered_slot_sum_kernel", 12)):         # (the slot sum lives in three translation units: gemm_tn, layernorm, embedding)
        rows = [e for e in table if sub in e["name"]]
        assert len(rows) == count, (sub, [e["name"] for e in rows])
        for e in rows:
            assert e["private_segment_fixed_size"] == 0 and e["vgpr_spill_count"] == 0 and e["sgpr_spill_count"] == 0, e
    # the ordered instance of the 64-row GEMM keeps the two-waves-per-SIMD budget of its default instance
    for e in table:
        if "gemm8t_kernel" in e["name"]:
            assert e["vgpr_count"] + e["agpr_count"] <= 256, e


def _bytes(fn, *args):
    n = ctypes.c_size_t(12345)
    return fn(*(args + (ctypes.byref(n),))), n.value


def test_workspace_sizes(lib):
    # 64-row kernel, 3 slices of a 264 x 520 product: 3 slabs + one column-sum row per (slice, j-tile); the general kernel (R = 96: three
    # chunks) caps 4 slices at 3; one slice: no slab, only the column-sum rows
    assert _bytes(lib.emdr2_gemm_tn_ordered_ws_bytes, 264, 520, 320, 3) == (0, (3 * 264 * 520 + 3 * 3 * 264) * 4)
    assert _bytes(lib.emdr2_gemm_tn_ordered_ws_bytes, 8, 8, 96, 4) == (0, (3 * 64 + 3 * 8) * 4)
    assert _bytes(lib.emdr2_gemm_tn_ordered_ws_bytes, 8, 8, 96, 2) == (0, (2 * 64 + 2 * 8) * 4)
    assert _bytes(lib.emdr2_gemm_tn_ordered_ws_bytes, 8, 8, 64, 5) == (0, (2 * 64 + 2 * 8) * 4)      # general kernel: 2; 64-row kernel: 1
    assert _bytes(lib.emdr2_gemm_tn_ordered_ws_bytes, 520, 8, 320, 1) == (0, 520 * 4)
    assert _bytes(lib.emdr2_layernorm_bwd_ordered_ws_bytes, 16391, 768) == (0, 2048 * 1536 * 4)
    assert _bytes(lib.emdr2_layernorm_bwd_ordered_ws_bytes, 9, 768) == (0, 2 * 1536 * 4)
    assert _bytes(lib.emdr2_layernorm_bwd_ordered_ws_bytes, 1000, 264) == (0, 32 * 2 * 264 * 4)
    # 641 tokens: 6 chunks of 128 with two piece slots each; 1 batch slice; 2 types
    assert _bytes(lib.emdr2_embedding_bwd_ordered_ws_bytes, 648, 81, 8, 32, 2) == (0, (6 * 2 * 32 + 8 * 32 + 8 * 2 * 32) * 4)
    assert _bytes(lib.emdr2_embedding_bwd_ordered_ws_bytes, 4097 * 8, 4097, 8, 32, 0) == (0, (257 * 2 * 32 + 16 * 8 * 32) * 4)


def test_argument_validation_needs_no_device(lib):
    p = ctypes.c_void_p(4096)                                         # never dereferenced: every call below returns before a launch
    n = ctypes.c_size_t()
    assert lib.emdr2_gemm_tn_ordered_ws_bytes(264, 520, 320, 3, None) == -1
    assert lib.emdr2_gemm_tn_ordered_ws_bytes(260, 520, 320, 3, ctypes.byref(n)) == -1            # I % 8
    assert lib.emdr2_gemm_tn_ordered_ws_bytes(264, 520, 330, 3, ctypes.byref(n)) == -1            # R % 32
    assert lib.emdr2_gemm_tn_ordered_ws_bytes(264, 520, 320, 0, ctypes.byref(n)) == -1
    g = lambda **kw: lib.emdr2_gemm_tn_bf16_ordered(kw.get("A", p), 264, kw.get("B", p), 520, kw.get("C", p), kw.get("ldc", 520), 264, 520,
                                                    kw.get("R", 320), kw.get("split", 3), kw.get("cs", None), kw.get("ws", p), kw.get("nws", 1 << 30), None)
    assert g(A=None) == -1 and g(B=None) == -1 and g(C=None) == -1 and g(R=330) == -1 and g(split=0) == -1 and g(ldc=512) == -1
    assert g(ws=None) == -1 and g(ws=ctypes.c_void_p(4100)) == -1
    assert g(nws=3 * 264 * 520 * 4 - 1) == -2 and g(cs=p, nws=3 * 264 * 520 * 4) == -2
    ln = lambda **kw: lib.emdr2_layernorm_bwd_ordered(kw.get("dy", p), p, p, p, p, None, p, kw.get("dg", p), p, kw.get("rows", 9), kw.get("H", 768),
                                                      kw.get("dmask", None), kw.get("p", 0.0), 0, kw.get("ws", p), kw.get("nws", 1 << 30), None)
    assert ln(dy=None) == -1 and ln(dg=None) == -1 and ln(rows=0) == -1 and ln(H=8193) == -1 and ln(ws=None) == -1
    assert ln(dmask=p, p=0.0) == -1 and ln(dmask=p, p=0.1, H=264) == -4 and ln(nws=2 * 1536 * 4 - 1) == -2
    assert lib.emdr2_layernorm_bwd_ordered_ws_bytes(0, 768, ctypes.byref(n)) == -1
    em = lambda **kw: lib.emdr2_embedding_bwd_ordered(kw.get("ids", p), kw.get("types", None), kw.get("cu", None), kw.get("nseq", 0), kw.get("order", p), p,
                                                      p, p, kw.get("dT", None), kw.get("tokens", 64), 8, 32, kw.get("nt", 0), kw.get("p", 0.0), 0,
                                                      kw.get("ws", p), kw.get("nws", 1 << 30), None)
    assert em(ids=None) == -1 and em(order=None) == -1 and em(ws=None) == -1 and em(p=1.0) == -1 and em(types=p) == -1 and em(cu=p, nseq=0) == -1
    assert em(tokens=63) == -4 and em(types=p, dT=p, nt=5) == -4 and em(nws=63) == -2
    assert lib.emdr2_embedding_bwd_ordered_ws_bytes(64, 0, 8, 32, 0, ctypes.byref(n)) == -1
