"""No GPU: --audit-index-interval parses, emdr2_mips_audit is declared, exported and bound with one arity and refuses bad arguments before
any launch, and the numpy restatement of the audit's sound words (tests/mips_audit_ref.py, the reference of tests/test_mips_audit_gpu.py)
says what it should on a hand-built 512 x 64 image with each premise of the search's proof broken in turn."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mips_audit_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ("--task OPENQA --num-layers 2 --hidden-size 128 --num-attention-heads 2 --max-position-embeddings 64 --seq-length 64 "
        "--decoder-seq-length 32 --batch-size 4 --lr 2e-4").split()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from emdr2_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        g.build()
    return _native.lib()


def test_audit_index_interval_flag():
    from emdr2_amd import arguments
    assert arguments.parse_args(BASE).audit_index_interval == 0                # off by default
    assert arguments.parse_args(BASE + ["--audit-index-interval", "25"]).audit_index_interval == 25
    with pytest.raises(ValueError, match="audit-index-interval"):
        arguments.parse_args(BASE + ["--audit-index-interval", "-1"])
    assert "--audit-index-interval" in arguments.get_parser().format_help()


def test_audit_symbol_is_declared_exported_and_bound_with_one_arity(lib):
    from emdr2_amd import _native
    text = open(os.path.join(ROOT, "include", "emdr2_mips.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+emdr2_mips_audit\s*\(([^)]*)\)", text)
    assert m, "include/emdr2_mips.h does not declare emdr2_mips_audit"
    n_args = len(m.group(1).split(","))
    assert n_args == 10
    assert re.search(r"#define\s+EMDR2_AUDIT_WORDS\s+16\b", text) and _native.AUDIT_WORDS == 16
    assert re.search(r"#define\s+EMDR2_ABI_VERSION\s+4\b", text)
    assert hasattr(lib, "emdr2_mips_audit"), "libemdr2_hip.so does not export emdr2_mips_audit"
    res, args = _native.SIGNATURES["emdr2_mips_audit"]
    assert res is ctypes.c_int and len(args) == n_args
    assert len(_native.AUDIT_NAMES) == 14 and len(set(_native.AUDIT_NAMES)) == 14
    # the names the header documents, in its order
    for i, name in enumerate(_native.AUDIT_NAMES):
        assert re.search(r"^\s*\*\s+%d\s+%s\b" % (i, name), open(os.path.join(ROOT, "include", "emdr2_mips.h")).read(), flags=re.M), name


def test_audit_rejects_bad_arguments_before_any_launch(lib):
    p = ctypes.c_void_p(4096)                                           # never dereferenced: every call below fails its validation
    call = lib.emdr2_mips_audit
    assert call(None, 10, 768, 0, p, None, None, None, p, None) == -1   # null image, emax_sq, report
    assert call(p, 10, 768, 0, None, None, None, None, p, None) == -1
    assert call(p, 10, 768, 0, p, None, None, None, None, None) == -1
    assert call(p, 10, 100, 0, p, None, None, None, p, None) == -1      # dim % 32, dim < 64
    assert call(p, 10, 32, 0, p, None, None, None, p, None) == -1
    assert call(p, -1, 768, 0, p, None, None, None, p, None) == -1
    assert call(p, 10, 768, 0, p, None, p, None, p, None) == -1         # shadow without table, table without shadow
    assert call(p, 10, 768, 0, p, None, None, p, p, None) == -1
    assert call(p, 10, 96, 0, p, None, p, p, p, None) == -1             # a shadow at a dim the seal does not take
    assert call(p, 10, 768, 0, p, None, p, ctypes.c_void_p(4100), p, None) == -1


# -- the numpy reference on a hand-built image --------------------------------------------------------------------------------------------
N, DIM, PADDED = 500, 64, 512


def _pack(rows, elem_bytes, elems_per_slot):
    """[512, 64] -> stripe-tiled bytes by the offset formula of DESIGN section 4, one slot at a time."""
    raw = np.ascontiguousarray(rows).view(np.uint8).reshape(PADDED, DIM * elem_bytes)
    per_chunk = 4 * elems_per_slot
    nch = DIM // per_chunk
    out = np.zeros(PADDED * DIM * elem_bytes, dtype=np.uint8)
    for row in range(PADDED):
        t, r = row >> 7, row & 127
        for c in range(nch):
            for s in range(4):
                off = ((t * nch) + c) * 8192 + (r * 4 + (s ^ ((r >> 2) & 3))) * 16
                k0 = (c * per_chunk + s * elems_per_slot) * elem_bytes
                out[off:off + 16] = raw[row, k0:k0 + 16]
    return out


def _world():
    rng = np.random.default_rng(5)
    rows = np.zeros((PADDED, DIM), dtype=np.float16)
    rows[:N] = (rng.standard_normal((N, DIM)) * rng.choice([0.25, 1.0, 4.0], size=(N, 1))).astype(np.float16)
    x = rows.astype(np.float64)
    n2 = (x * x).sum(axis=1)
    emax = np.float32(n2.max() * 1.0000001)
    norms = np.array([n2[:256].max(), n2[256:].max()]) * 1.0000001
    table = np.zeros((2, 4), dtype=np.float32)
    e8 = np.zeros((PADDED, DIM), dtype=np.int8)
    for b in range(2):
        blk = x[b * 256:(b + 1) * 256]
        s = np.float32(np.abs(blk).max() / 127.0)
        q = np.clip(np.rint(blk / np.float64(s)), -127, 127)
        e8[b * 256:(b + 1) * 256] = q
        resid = np.sqrt(((blk - np.float64(s) * q) ** 2).sum(axis=1)).max()
        table[b] = (s, np.sqrt(n2[b * 256:(b + 1) * 256].max()) * 1.001, resid * 1.001, 0.0)
    return dict(rows=rows, e8=e8, emax=emax, norms=norms.astype(np.float32), table=table, n2=n2)


def _run(w, **over):
    a = dict(w, **over)
    return ref.sound_reference(_pack(a["rows"], 2, 8), N, DIM, 1000, float(a["emax"]), a["norms"], _pack(a["e8"], 1, 16), a["table"])


def test_layout_restatement_inverts_the_offset_formula():
    w = _world()
    assert np.array_equal(ref.tiled_rows_bits(_pack(w["rows"], 2, 8), DIM), w["rows"].view(np.uint16))
    assert np.array_equal(ref.shadow_rows(_pack(w["e8"], 1, 16), DIM), w["e8"])


def test_reference_is_clean_on_a_consistent_image_and_flags_each_broken_premise():
    w = _world()
    clean = _run(w)
    assert clean == {0: N, 1: 0, 2: 0, 3: 0, 4: 0, 7: 0, 8: 0, 9: 0, 12: ref.NONE}
    norm = np.sqrt(w["n2"][:N])

    rows = w["rows"].copy(); rows[505, 3] = np.float16(-0.0)            # a padding row with one bit set: bits are checked, not values
    got = _run(w, rows=rows)
    assert got == {**clean, **{1: 1, 12: 1505}}

    e8 = w["e8"].copy(); e8[511, 63] = 1
    assert _run(w, e8=e8) == {**clean, **{7: 1, 12: 1511}}

    got = _run(w, emax=np.float32(w["emax"] * 0.5))
    want = int((norm > np.float64(np.sqrt(np.float32(w["emax"] * 0.5)) * np.float32(1.001))).sum())
    assert want >= 1 and got[3] == want and got[4] == got[8] == got[9] == 0
    assert got[12] == 1000 + int(np.nonzero(norm > np.float64(np.sqrt(np.float32(w["emax"] * 0.5)) * np.float32(1.001)))[0][0])

    norms = w["norms"].copy(); norms[1] *= 0.5
    got = _run(w, norms=norms)
    want = int((w["n2"][256:N] > np.float64(norms[1]) * 1.001 * 1.001).sum())
    assert want >= 1 and got[4] == want and got[3] == 0 and got[12] >= 1256

    for col, word in ((1, 8), (2, 9), (0, 9)):                          # N_b halved, D_b halved, s_b doubled
        table = w["table"].copy(); table[0, col] *= 2.0 if col == 0 else 0.5
        got = _run(w, table=table)
        assert got[word] >= 1 and got[12] < 1256, (col, got)
        assert all(got[k] == 0 for k in (1, 2, 3, 4, 7)), (col, got)

    rows = w["rows"].copy(); rows[7, 0] = np.float16(np.inf); rows[300, 5] = np.float16(np.nan)
    got = _run(w, rows=rows)                                             # non-finite rows: counted once, left out of 3, 4, 8, 9
    assert got == {**clean, **{2: 2, 12: 1007}}

    assert ref.sound_reference(np.zeros(512 * 64 * 2, dtype=np.uint8), 0, DIM, 0, 0.0)[12] == ref.NONE
