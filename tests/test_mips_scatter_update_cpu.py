"""No GPU: the scattered-update entries of include/emdr2_mips.h validate their arguments before any launch, the duplicate resolution of
`update_rows_at` (last occurrence wins) agrees with a dict restatement, the retriever's doc-id -> row matching does what it says, and
--index-writeback has its two rules."""
import ctypes
import os

import numpy as np
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from emdr2_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        g.build()
    return _native.lib()


def _ws_bytes(lib, n_rows, n_upd):
    n = ctypes.c_size_t()
    assert lib.emdr2_mips_scatter_workspace_bytes(n_rows, n_upd, ctypes.byref(n)) == 0
    return n.value


def test_scatter_workspace_bytes(lib):
    n = ctypes.c_size_t()
    assert lib.emdr2_mips_scatter_workspace_bytes(1000, 10, None) == -1
    assert lib.emdr2_mips_scatter_workspace_bytes(-1, 10, ctypes.byref(n)) == -1
    assert lib.emdr2_mips_scatter_workspace_bytes(1000, -1, ctypes.byref(n)) == -1
    # grows with both arguments: a claim word per 256-row block of the padded image, a list entry per row up to one per block
    assert _ws_bytes(lib, 1000, 1) < _ws_bytes(lib, 1000, 3) < _ws_bytes(lib, 1000, 4) == _ws_bytes(lib, 1000, 4000)
    assert _ws_bytes(lib, 1000, 3) < _ws_bytes(lib, 100_000, 3) < _ws_bytes(lib, 21_015_324, 3)
    assert _ws_bytes(lib, 21_015_324, 3200) < _ws_bytes(lib, 21_015_324, 25_600)
    blocks = (21_015_324 + 511) // 512 * 2
    assert 4 * blocks + 4 * 3200 <= _ws_bytes(lib, 21_015_324, 3200) <= 4 * blocks + 4 * 3200 + 64
    assert _ws_bytes(lib, 1000, 0) > 0                                  # (the claim words alone)


def test_scattered_update_rejects_bad_arguments_before_any_launch(lib):
    p = ctypes.c_void_p(4096)                                           # never dereferenced: every call below fails its validation
    big = 1 << 20
    call = lib.emdr2_mips_update_rows_scattered
    # null pointers: rows, ids, image, block-norm table, emax_sq, workspace
    assert call(None, p, 10, 768, 1000, p, p, p, None, None, None, p, big, None) == -1
    assert call(p, None, 10, 768, 1000, p, p, p, None, None, None, p, big, None) == -1
    assert call(p, p, 10, 768, 1000, None, p, p, None, None, None, p, big, None) == -1
    assert call(p, p, 10, 768, 1000, p, None, p, None, None, None, p, big, None) == -1
    assert call(p, p, 10, 768, 1000, p, p, None, None, None, None, p, big, None) == -1
    assert call(p, p, 10, 768, 1000, p, p, p, None, None, None, None, big, None) == -1
    # a shadow image without its table / its flag, a misaligned table, a shadow at a dim the seal does not take
    assert call(p, p, 10, 768, 1000, p, p, p, p, None, p, p, big, None) == -1
    assert call(p, p, 10, 768, 1000, p, p, p, p, p, None, p, big, None) == -1
    assert call(p, p, 10, 768, 1000, p, p, p, p, ctypes.c_void_p(4100), p, p, big, None) == -1
    assert call(p, p, 10, 96, 1000, p, p, p, p, p, p, p, big, None) == -1
    # bad dim, bad counts
    assert call(p, p, 10, 100, 1000, p, p, p, None, None, None, p, big, None) == -1
    assert call(p, p, 10, 32, 1000, p, p, p, None, None, None, p, big, None) == -1
    assert call(p, p, -1, 768, 1000, p, p, p, None, None, None, p, big, None) == -1
    assert call(p, p, 10, 768, -1, p, p, p, None, None, None, p, big, None) == -1
    # a workspace one byte short
    need = _ws_bytes(lib, 1000, 10)
    assert call(p, p, 10, 768, 1000, p, p, p, None, None, None, p, need - 1, None) == -2
    assert call(p, p, 10, 768, 1000, p, p, p, p, p, p, p, need - 1, None) == -2
    # nothing to do is not an error (and launches nothing)
    assert call(p, p, 0, 768, 1000, p, p, p, None, None, None, p, big, None) == 0


def _last_wins(ids):
    last = {}
    for i, r in enumerate(ids):
        last[r] = i
    return [r if last[r] == i else -1 for i, r in enumerate(ids)]


def test_duplicate_resolution_keeps_the_last_occurrence():
    from emdr2_amd.data.emdr2_index import resolve_duplicate_rows
    rng = np.random.default_rng(3)
    fixed = [[5], [-1], [7, 1, 7, 2, 7, 3], [-1, 4, -1, 4, -1], [9, 9, 9, 9], [3, 2, 1, 0], [1 << 40, 5, 1 << 40, -(1 << 40), 5, -(1 << 40)]]
    lists = fixed + [rng.integers(-1, max(2, n // 3), size=n).tolist() for n in rng.integers(1, 400, size=200)]
    for ids in lists:
        got = resolve_duplicate_rows(torch.tensor(ids, dtype=torch.int64))
        want = _last_wins(ids)
        # -1 is "skip" whichever way it got there, so an original -1 that the dict keeps as the last -1 is simply -1 in both
        assert got.tolist() == want, ids
    out = resolve_duplicate_rows(torch.tensor([7, 1, 7, 2, 7, 3]))
    assert out.tolist() == [-1, 1, -1, 2, 7, 3] and out.dtype == torch.int64


def test_kept_rows_match_kept_doc_ids_against_the_question_s_own_search():
    from emdr2_amd.model.emdr2_model import kept_rows
    searched_ids = torch.tensor([[11, 12, 13, 14, 15], [12, 11, 30, -1, -1], [40, 41, 42, 43, 44]], dtype=torch.int32)
    searched_rows = torch.tensor([[100, 101, 102, 103, 104], [101, 100, 250, -1, -1], [7, 6, 5, 4, 3]], dtype=torch.int64)
    kept = torch.tensor([[11, 13, 14, 15], [12, 11, 30, -1], [40, 41, 42, 43]], dtype=torch.int32)    # trivial doc 12 dropped / empty slot / surplus slot
    got = kept_rows(kept, searched_ids, searched_rows)
    assert got.tolist() == [[100, 102, 103, 104], [101, 100, 250, -1], [7, 6, 5, 4]] and got.dtype == torch.int64


BASE = ("--task OPENQA --num-layers 2 --hidden-size 128 --num-attention-heads 2 --max-position-embeddings 64 --seq-length 64 "
        "--decoder-seq-length 32 --batch-size 4 --lr 2e-4").split()


def test_index_writeback_flag_and_its_rules():
    from emdr2_amd import arguments
    assert arguments.parse_args(BASE).index_writeback is False            # off by default
    # the two legal combinations: without a refresher, and next to the rolling one
    assert arguments.parse_args(BASE + ["--index-writeback", "--disable-retriever-dropout"]).index_writeback is True
    args = arguments.parse_args(BASE + ["--index-writeback", "--disable-retriever-dropout", "--async-indexer", "--index-refresh-in-place"])
    assert args.index_writeback and args.index_refresh_in_place
    # a training-mode tower would write dropout noise into the index
    with pytest.raises(ValueError, match="disable-retriever-dropout"):
        arguments.parse_args(BASE + ["--index-writeback"])
    # swap mode: a refresh is always in progress and every write would be discarded at the next commit
    with pytest.raises(ValueError, match="index-refresh-in-place"):
        arguments.parse_args(BASE + ["--index-writeback", "--disable-retriever-dropout", "--async-indexer"])
    help_text = " ".join(arguments.get_parser().format_help().split())
    for phrase in ("--index-writeback", "whatever was written LAST", "rolling refresher", "semantics, not a tuning knob"):
        assert phrase in help_text, phrase
