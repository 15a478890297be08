"""GPU: the index audit (emdr2_mips_audit, HipIndexShard.audit, DistributedBruteForceIndex.audit, --audit-index-interval).

Clean states report zero after every writer of the derived structures; each planted fault -- a value written inside an allocated tensor,
nothing else -- makes the device report equal the host reference (tests/mips_audit_ref.py: numpy float64 for the sound words, a fresh
run of the project's seal / block-norm entries for the canonical ones) word for word, with the words the fault is about non-zero; after
the value is restored the audit is clean again.  Shapes are the smallest at which each mechanism exists: 9,000 x 256 with a shadow (36
blocks, the last holds 40 real rows and 216 padding rows), 8,492 x 768 with a shadow, 300 x 96 (no shadow possible), 0 rows."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mips_audit_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = (1 << 64) - 1
SHAPES = {"9000x256": (9000, 256), "8492x768": (8492, 768), "300x96": (300, 96)}
SHADOWED = ("9000x256", "8492x768")
_ROWS = {}


@pytest.fixture(scope="module")
def lib():
    from emdr2_amd import _native
    return _native.lib()


def _rows(shape, kind="normal"):
    """fp16 [n, dim], made once per (shape, kind) and never modified: N(0,1) x mixed magnitudes, or ternary rows (the seal's d2 == 0 case)."""
    if (shape, kind) not in _ROWS:
        n, d = SHAPES[shape]
        rng = np.random.default_rng(n + d)
        if kind == "ternary":
            r = rng.integers(-1, 2, size=(n, d)).astype(np.float16)
        else:
            r = (rng.standard_normal((n, d)) * rng.choice([0.05, 1.0, 8.0], size=(n, 1))).astype(np.float16)
        r.setflags(write=False)
        _ROWS[(shape, kind)] = r
    return _ROWS[(shape, kind)]


def _shard(shape, kind="normal", row_base=0):
    from emdr2_amd.data.emdr2_index import HipIndexShard
    n, d = SHAPES[shape]
    sh = HipIndexShard(d, n, row_base, shadow_min_rows=256)
    sh.append_rows(np.array(_rows(shape, kind)))
    assert (sh._shadow is not None) == (shape in SHADOWED)
    return sh


def _words(result):
    from emdr2_amd import _native
    return [result[n] for n in _native.AUDIT_NAMES]


def _assert_clean(sh):
    a = sh.audit()
    assert _words(a) == [sh.n_rows] + [0] * 11 + [NONE, NONE], a
    assert a["sound"] is True and a["canonical"] is True and a["shadow_in_use"] is (sh._shadow is not None)
    return a


def _assert_matches_reference(lib, sh):
    a = sh.audit()
    want = ref.full_reference(lib, sh)
    print("device", _words(a), "reference", want)
    assert _words(a) == want
    return a


def _build_table(sh, shape):
    """the block-norm table exists after the first in-place update: rewrite row 0 with itself"""
    sh.update_rows(0, torch.from_numpy(np.array(_rows(shape)[0:1])).to(sh.device))
    assert sh._block_norms is not None


# byte offsets inside the images, restated from DESIGN section 4
def _off16(row, k, dim):
    nch = dim // 32
    t, r, c, s, e = row >> 7, row & 127, k // 32, (k % 32) // 8, k % 8
    return ((t * nch + c) * 512 + r * 4 + (s ^ ((r >> 2) & 3))) * 16 + e * 2


def _off8(row, k, dim):
    nch8 = dim // 64
    t, r, c, s, e = row >> 7, row & 127, k // 64, (k % 64) // 16, k % 16
    return ((t * nch8 + c) * 512 + r * 4 + (s ^ ((r >> 2) & 3))) * 16 + e


def _half(sh, row, k):
    """a one-element int16 view of fp16 element k of image row `row` (inside the allocated image: row < padded rows)"""
    assert 0 <= row < (max(sh.n_rows, 1) + 511) // 512 * 512 and 0 <= k < sh.dim
    i = _off16(row, k, sh.dim) // 2
    return sh.tiled.view(torch.int16)[i:i + 1]


def _byte(sh, row, k):
    assert 0 <= row < (sh.n_rows + 255) // 256 * 256 and 0 <= k < sh.dim
    i = _off8(row, k, sh.dim)
    return sh._shadow[0].view(torch.int8)[i:i + 1]


# -- 1. clean states ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_clean_after_every_writer(lib, shape):
    n, d = SHAPES[shape]
    sh = _shard(shape)
    _assert_clean(sh)
    _assert_matches_reference(lib, sh)
    rng = np.random.default_rng(1)
    new = lambda m: torch.from_numpy((rng.standard_normal((m, d)) * 3.0).astype(np.float16)).to(sh.device)
    sh.update_rows(250, new(20))                                        # crosses the boundary of blocks 0 and 1
    _assert_clean(sh)
    sh.update_rows(n - 30, new(30))                                     # ends in the last, partial block
    _assert_clean(sh)
    assert sh._block_norms is not None
    ids = torch.tensor([5, n - 1, 5, -1, n, n + 100, 1 << 40, 257, 5, n - 1], dtype=torch.int64, device=sh.device)   # duplicates, out of range
    sh.update_rows_at(ids, new(ids.numel()))
    _assert_clean(sh)
    _assert_matches_reference(lib, sh)
    sh.begin_refresh()
    sh.refresh_rows(0, new(n // 2))
    _assert_clean(sh)                                                   # mid-refresh: the image being searched, not the half-written spare
    sh.refresh_rows(n // 2, new(n - n // 2))
    sh.commit_refresh()
    assert sh._block_norms is None
    _assert_clean(sh)
    _assert_matches_reference(lib, sh)


def test_clean_on_an_empty_shard_and_on_ternary_rows(lib):
    from emdr2_amd.data.emdr2_index import HipIndexShard
    empty = HipIndexShard(256, 0, 0)
    a = empty.audit()
    assert _words(a) == [0] * 12 + [NONE, NONE] and a["sound"] and a["canonical"] and not a["shadow_in_use"]
    for shape in SHADOWED:
        sh = _shard(shape, "ternary")
        _assert_clean(sh)
        _assert_matches_reference(lib, sh)
        assert float(sh._shadow[1].view(-1, 4)[:(sh.n_rows + 255) // 256, 2].min()) > 0.0   # D_b carries the 2^-22 N_b term although d2 == 0


def test_a_partly_filled_shard_raises_like_search():
    from emdr2_amd.data.emdr2_index import HipIndexShard
    sh = HipIndexShard(96, 300, 0)
    sh.append_rows(np.array(_rows("300x96")[:100]))
    with pytest.raises(RuntimeError, match=r"shard not fully populated \(100 of 300 rows\)"):
        sh.audit()


@pytest.mark.parametrize("shape", ["9000x256", "300x96"])
def test_clean_after_a_snapshot_round_trip_and_a_failing_audit_refuses_the_load(shape, tmp_path, monkeypatch):
    from emdr2_amd.data.emdr2_index import DistributedBruteForceIndex, HipIndexShard
    n, d = SHAPES[shape]
    monkeypatch.setattr(DistributedBruteForceIndex, "_make_shard", lambda self, dim, n_rows, row_base: HipIndexShard(dim, n_rows, row_base, shadow_min_rows=256))
    index = DistributedBruteForceIndex(d, None, use_gpu=True)
    index.add_arrays(np.arange(1, n + 1, dtype=np.int32), np.array(_rows(shape)))
    path = str(tmp_path / "index.flat")
    index.save_flat_file(path)
    other = DistributedBruteForceIndex(d, None, use_gpu=True)
    other.load_flat_snapshot(path, audit=True)
    a = other.audit()
    assert a["sound"] and a["canonical"] and a["rows_checked"] == n and a["shadow_in_use"] is (shape in SHADOWED)
    # the digest covers the fp16 rows only: a loader that left emax_sq low would pass it, and not the audit
    inner = DistributedBruteForceIndex.add_flat_file

    def low_emax(self, flat):
        inner(self, flat)
        self.shard.emax_sq.mul_(0.5)
    monkeypatch.setattr(DistributedBruteForceIndex, "add_flat_file", low_emax)
    third = DistributedBruteForceIndex(d, None, use_gpu=True)
    third.load_flat_snapshot(path)                                      # without the audit: accepted
    with pytest.raises(ValueError, match="rows_over_emax"):
        DistributedBruteForceIndex(d, None, use_gpu=True).load_flat_snapshot(path, audit=True)


# -- 2. planted faults ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fault_a_nonzero_half_in_a_padding_row(lib, shape):
    n, d = SHAPES[shape]
    sh = _shard(shape, row_base=70000)
    cell = _half(sh, n + 5, 3)
    cell.fill_(1)                                                       # the smallest subnormal
    a = _assert_matches_reference(lib, sh)
    assert a["pad_rows_nonzero"] == 1 and a["first_bad_row"] == 70000 + n + 5 and a["sound"] is False
    cell.fill_(0)
    _assert_clean(sh)


@pytest.mark.parametrize("shape", SHADOWED)
def test_fault_b_nonzero_byte_in_a_padding_row_of_the_int8_image(lib, shape):
    n, d = SHAPES[shape]
    sh = _shard(shape)
    cell = _byte(sh, n + 7, d - 1)
    cell.fill_(1)
    a = _assert_matches_reference(lib, sh)
    assert a["shadow_pad_rows_nonzero"] == 1 and a["pad_rows_nonzero"] == 0 and a["first_bad_row"] == n + 7 and a["sound"] is False
    cell.fill_(0)
    _assert_clean(sh)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fault_c_emax_sq_too_low(lib, shape):
    sh = _shard(shape)
    old = sh.emax_sq.clone()
    sh.emax_sq.mul_(0.99)
    a = _assert_matches_reference(lib, sh)
    assert a["rows_over_emax"] >= 1 and a["emax_noncanonical"] == 1 and not a["sound"] and not a["canonical"]
    sh.emax_sq.copy_(old)
    _assert_clean(sh)


def _plant_with_pack_rows(lib, sh, row, values):
    """the misuse the API allows: a row written into the LIVE image with emdr2_mips_pack_rows (emax_sq of its own), not update_rows"""
    from emdr2_amd import _native
    scratch = torch.zeros(1, dtype=torch.float32, device=sh.device)
    v = values.contiguous()
    assert 0 <= row < sh.n_rows and tuple(v.shape) == (1, sh.dim) and v.dtype == torch.float16
    _native.check(lib.emdr2_mips_pack_rows(v.data_ptr(), 1, sh.dim, row, sh.n_rows, sh.tiled.data_ptr(), scratch.data_ptr(), _native.stream_ptr()), "pack_rows")


def _big_row(shape, sh):
    rows = _rows(shape)
    worst = int(np.argmax((rows.astype(np.float64) ** 2).sum(axis=1)))
    return torch.from_numpy(np.array(rows[worst:worst + 1]) * np.float16(4.0)).to(sh.device)


@pytest.mark.parametrize("shape", SHADOWED)
def test_fault_d_a_large_row_written_behind_the_tables_back(lib, shape):
    sh = _shard(shape)
    row = 512                                                           # the first row of block 2
    old = sh.rows([row]).clone()
    big = _big_row(shape, sh)
    _plant_with_pack_rows(lib, sh, row, big)
    a = _assert_matches_reference(lib, sh)
    assert a["rows_over_emax"] >= 1 and a["shadow_norm_low"] >= 1 and a["shadow_rows_noncanonical"] >= 1 and a["block_norm_low"] == 0
    assert a["first_bad_row"] == row and not a["sound"]
    _plant_with_pack_rows(lib, sh, row, old)
    _assert_clean(sh)
    _build_table(sh, shape)
    _assert_clean(sh)
    _plant_with_pack_rows(lib, sh, row, big)
    a = _assert_matches_reference(lib, sh)
    assert a["rows_over_emax"] >= 1 and a["block_norm_low"] >= 1 and a["shadow_norm_low"] >= 1 and a["shadow_rows_noncanonical"] >= 1
    assert a["block_norm_noncanonical"] == 1 and a["first_bad_row"] == row and a["first_bad_block"] == 2
    _plant_with_pack_rows(lib, sh, row, old)
    _assert_clean(sh)


def _residuals(sh, block):
    """float64 ||e_r - s_b e8_r|| of the 256 rows of `block`, and the block's int8 rows, from the stored buffers"""
    x = ref.tiled_rows_bits(sh.tiled.cpu().numpy(), sh.dim)[block * 256:(block + 1) * 256].view(np.float16).astype(np.float64)
    e8 = ref.shadow_rows(sh._shadow[0].cpu().numpy(), sh.dim)[block * 256:(block + 1) * 256]
    s = float(sh._shadow[1].view(-1, 4)[block, 0])
    r = x - s * e8.astype(np.float64)
    return np.sqrt((r * r).sum(axis=1)), e8


@pytest.mark.parametrize("shape", SHADOWED)
def test_faults_e_f_one_int8_byte_off(lib, shape):
    sh = _shard(shape)
    block = 3
    resid, e8 = _residuals(sh, block)
    # (e) +1 on a byte of the row with the SMALLEST residual: canonical drift, the proof's premise intact
    r = int(np.argmin(resid))
    k = int(np.argmax(e8[r] < 100))
    cell = _byte(sh, block * 256 + r, k)
    cell.fill_(int(e8[r, k]) + 1)
    a = _assert_matches_reference(lib, sh)
    assert a["shadow_rows_noncanonical"] == 1 and a["shadow_resid_low"] == 0 and a["sound"] is True and a["canonical"] is False
    assert a["first_bad_row"] == block * 256 + r
    cell.fill_(int(e8[r, k]))
    _assert_clean(sh)
    # (f) +64 on a byte of the row with the LARGEST residual
    r = int(np.argmax(resid))
    k = int(np.argmax(e8[r] <= 0))
    cell = _byte(sh, block * 256 + r, k)
    cell.fill_(int(e8[r, k]) + 64)
    a = _assert_matches_reference(lib, sh)
    assert a["shadow_resid_low"] >= 1 and a["shadow_rows_noncanonical"] == 1 and a["sound"] is False
    cell.fill_(int(e8[r, k]))
    _assert_clean(sh)


@pytest.mark.parametrize("shape", SHADOWED)
def test_fault_g_block_constants_of_the_shadow_table(lib, shape):
    sh = _shard(shape)
    block = 3
    entry = sh._shadow[1].view(-1, 4)[block]
    for col, factor, word in ((1, 0.5, "shadow_norm_low"), (2, 0.5, "shadow_resid_low"), (0, 2.0, "shadow_resid_low")):   # N_b, D_b, s_b
        old = entry[col].clone()
        entry[col] = old * factor
        a = _assert_matches_reference(lib, sh)
        assert a[word] >= 1 and a["shadow_table_noncanonical"] == 1 and a["first_bad_block"] == block and not a["sound"], (col, a)
        entry[col] = old
        _assert_clean(sh)


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_fault_h_a_block_norm_entry_too_low(lib, shape):
    sh = _shard(shape)
    _build_table(sh, shape)
    _assert_clean(sh)
    block = 1
    old = sh._block_norms[block].clone()
    sh._block_norms[block] = old * 0.5
    a = _assert_matches_reference(lib, sh)
    assert a["block_norm_low"] >= 1 and a["block_norm_noncanonical"] == 1 and a["emax_noncanonical"] == 0 and a["first_bad_block"] == block
    sh._block_norms[block] = old
    _assert_clean(sh)


@pytest.mark.parametrize("shape", SHADOWED)
def test_fault_i_an_inf_under_a_shadow_in_use(lib, shape):
    sh = _shard(shape)
    cell = _half(sh, 100, 0)
    old = cell.clone()
    cell.fill_(0x7c00)                                                  # +inf
    a = _assert_matches_reference(lib, sh)                              # (the reference leaves the row out of words 3, 4, 8, 9)
    assert a["nonfinite_rows"] == 1 and a["shadow_in_use"] is True and a["sound"] is False
    assert a["rows_over_emax"] == 0 and a["shadow_norm_low"] == 0 and a["shadow_resid_low"] == 0 and a["first_bad_row"] <= 100
    cell.copy_(old)
    _assert_clean(sh)


def test_an_inf_without_a_shadow_is_counted_but_sound(lib):
    sh = _shard("300x96")
    cell = _half(sh, 100, 0)
    old = cell.clone()
    cell.fill_(0x7c00)
    a = _assert_matches_reference(lib, sh)
    assert a["nonfinite_rows"] == 1 and a["shadow_in_use"] is False and a["sound"] is True
    cell.copy_(old)
    _assert_clean(sh)


# -- 3. sound really means wrong ------------------------------------------------------------------------------------------------------------
def test_a_flagged_state_and_the_search_after_the_proper_update(lib):
    shape = "9000x256"
    n, d = SHAPES[shape]
    sh = _shard(shape)
    row, k = 8700, 10                                                   # behind the dense first segment: on the int8 segment
    big = _big_row(shape, sh)
    rng = np.random.default_rng(2)
    q = rng.standard_normal((129, d)).astype(np.float16)
    q[0] = (big.cpu().numpy()[0].astype(np.float32) / 64.0).astype(np.float16)       # the planted row is query 0's best match
    q = torch.from_numpy(q).to(sh.device)
    _plant_with_pack_rows(lib, sh, row, big)
    a = sh.audit()
    assert a["sound"] is False and a["rows_over_emax"] >= 1 and a["shadow_norm_low"] >= 1
    fast = sh.search(q, k, exact_fallback=False)                        # may or may not be right: nothing is asserted about it
    sel = torch.arange(129, dtype=torch.int32, device=sh.device)

    def exact():
        dist = torch.empty((129, k), dtype=torch.float16, device=sh.device)
        idx = torch.empty((129, k), dtype=torch.int32, device=sh.device)
        rows = torch.empty((129, k), dtype=torch.int64, device=sh.device)
        flags = torch.zeros(129, dtype=torch.int32, device=sh.device)
        sh.search_exact(q, sel, k, dist, idx, rows, flags)
        return dist, idx, rows
    truth = exact()
    assert int(truth[2][0, 0]) == row
    print("with the fault in place the fast path %s the exact one" % ("equals" if all(torch.equal(x, y) for x, y in zip(fast[:3], truth)) else "differs from"))
    sh.update_rows(row, big)                                            # the same row, written properly
    _assert_clean(sh)
    fast = sh.search(q, k, exact_fallback=False)
    truth = exact()
    proven = fast[3] == 0                                               # (a query the fast path could not prove is the exact path's to answer)
    assert bool(proven[0]) and int(proven.sum()) >= 100
    for x, y in zip(fast[:3], truth):
        assert torch.equal(x[proven], y[proven])
    assert int(fast[2][0, 0]) == row


# -- 4. ABI ---------------------------------------------------------------------------------------------------------------------------------
def test_abi_return_codes_on_real_buffers(lib):
    from emdr2_amd import _native
    sh = _shard("9000x256")
    report = torch.full((16,), 7, dtype=torch.int64, device=sh.device)
    t, e, r, s = sh.tiled.data_ptr(), sh.emax_sq.data_ptr(), report.data_ptr(), _native.stream_ptr()
    image, table = sh._shadow[0].data_ptr(), sh._shadow[1].data_ptr()
    assert lib.emdr2_mips_audit(None, 9000, 256, 0, e, None, None, None, r, s) == -1
    assert lib.emdr2_mips_audit(t, 9000, 256, 0, None, None, None, None, r, s) == -1
    assert lib.emdr2_mips_audit(t, 9000, 256, 0, e, None, None, None, None, s) == -1
    assert lib.emdr2_mips_audit(t, 9000, 100, 0, e, None, None, None, r, s) == -1
    assert lib.emdr2_mips_audit(t, 9000, 256, 0, e, None, image, None, r, s) == -1
    torch.cuda.synchronize()
    assert report.tolist() == [7] * 16                                  # a refused call launches nothing
    assert lib.emdr2_mips_audit(t, 0, 256, 0, e, None, None, None, r, s) == 0
    assert [w & NONE for w in report.tolist()] == [0] * 12 + [NONE, NONE, 0, 0]
    assert lib.emdr2_mips_audit(t, 9000, 256, 0, e, None, image, table, r, s) == 0
    assert [w & NONE for w in report.tolist()] == [9000] + [0] * 11 + [NONE, NONE, 0, 0]           # the reserved words are left 0


# -- 5. sharded -----------------------------------------------------------------------------------------------------------------------------
def _sharded_worker(rank, world, port):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_dist_gpu import _init
    _init(rank, world, port, "gloo")
    from emdr2_amd.data.emdr2_index import DistributedBruteForceIndex, FaissMIPSIndex
    n, d = SHAPES["9000x256"]
    rows = np.array(_rows("9000x256"))
    index = DistributedBruteForceIndex(d, None, use_gpu=True)
    index.add_arrays(np.arange(1, n + 1, dtype=np.int32), rows)
    assert index.local_rows() == ((0, 4500) if rank == 0 else (4500, 9000))

    def same_everywhere(result):
        got = [None, None]
        torch.distributed.all_gather_object(got, result)
        assert got[0] == got[1] == result, got
    clean = index.audit()
    same_everywhere(clean)
    assert [clean[k] for k in clean if k not in ("sound", "canonical", "shadow_in_use")] == [9000] + [0] * 11 + [NONE, NONE]
    assert clean["sound"] and clean["canonical"] and not clean["shadow_in_use"]
    if rank == 1:                                                       # fault (a) on rank 1 only: a padding row of its shard
        i = _off16(4500 + 5, 3, d) // 2
        index.shard.tiled.view(torch.int16)[i:i + 1].fill_(1)
    bad = index.audit()
    same_everywhere(bad)
    assert bad["pad_rows_nonzero"] == 1 and bad["first_bad_row"] == 4500 + 4505 and not bad["sound"] and bad["rows_checked"] == 9000
    assert callable(FaissMIPSIndex.audit) and FaissMIPSIndex.audit is DistributedBruteForceIndex.audit
    torch.distributed.destroy_process_group()


def test_two_ranks_return_the_same_reduced_report():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_sharded_worker, args=(2, port), nprocs=2, join=True)


# -- 6. the loop's hook ---------------------------------------------------------------------------------------------------------------------
def test_step_boundary_hook_audits_on_the_interval_and_raises_on_every_failure(monkeypatch, capsys):
    from emdr2_amd.data.emdr2_index import DistributedBruteForceIndex
    from emdr2_amd.tasks.openqa.e2eqa.train_e2eqa import maybe_audit_index
    n, d = SHAPES["300x96"]
    index = DistributedBruteForceIndex(d, None, use_gpu=True)
    index.add_arrays(np.arange(1, n + 1, dtype=np.int32), np.array(_rows("300x96")))
    calls = []
    inner = DistributedBruteForceIndex.audit

    def counted(self):
        calls.append(1)
        return inner(self)
    monkeypatch.setattr(DistributedBruteForceIndex, "audit", counted)
    assert [maybe_audit_index(index, it, 2) for it in range(5)] == [True, False, True, False, True] and len(calls) == 3
    out = capsys.readouterr().out
    assert [int(m) for m in re.findall(r"index audit at iteration (\d+): 300 rows, sound, canonical \(\d+\.\d\d ms\)", out)] == [0, 2, 4]
    assert [maybe_audit_index(index, it, 0) for it in range(5)] == [False] * 5 and len(calls) == 3
    cell = _half(index.shard, n + 5, 3)
    cell.fill_(1)
    with pytest.raises(RuntimeError, match="pad_rows_nonzero"):
        maybe_audit_index(index, 4, 2)
    assert maybe_audit_index(index, 5, 2) is False                      # not on the interval: not looked at
    out = capsys.readouterr().out
    assert "index audit at iteration 4: 300 rows, FAILED: pad_rows_nonzero=1" in out and "first_bad_row=305" in out
    cell.fill_(0)
    assert maybe_audit_index(index, 6, 2) is True


# -- 7. the task --------------------------------------------------------------------------------------------------------------------------------
def test_task_run_audits_before_the_first_step_and_at_every_boundary(tmp_path, capsys):
    from test_task_gpu import _argv, _make_world
    from emdr2_amd import checkpointing
    from emdr2_amd.tasks import run as task_run
    tmp = str(tmp_path)
    vocab, ev, emb = _make_world(tmp, n_train=12)                       # 12 questions / batch 4: three steps
    argv = _argv(tmp, vocab, ev, emb, extra=("--index-refresh-in-place", "--index-writeback", "--disable-retriever-dropout",
                                              "--audit-index-interval", "1"))
    task_run.main(argv)
    out = capsys.readouterr().out
    assert checkpointing.read_tracker(os.path.join(tmp, "ckpt"))[0] == 3
    audits = re.findall(r"index audit at iteration (\d+): 300 rows, sound, canonical", out)
    assert [int(a) for a in audits] == [0, 1, 2, 3], out[-2000:]
    assert "FAILED" not in out
