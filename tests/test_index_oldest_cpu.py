"""CPU: the oldest-first row selection (emdr2_mips_oldest_rows, HipIndexShard.oldest_rows, --index-refresh-oldest-first).  The numpy
statement of the contract in include/emdr2_mips.h that tests/test_index_oldest_gpu.py compares the device with, its own properties, the
argument validation of the two C entries, the flag's rules, and the refresher's bookkeeping on a stub index whose selection is the numpy
one."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_index_generations_cpu import BASE, U64_NONE, _builder

INFO_NAMES = ("n_selected", "n_eligible", "max_stamp_selected", "reserved")


def oldest_rows_reference(stamps, n, below, row_base=0):
    """-> (out_rows int64 [n], [n_selected, n_eligible, largest stamp selected or 2^64 - 1, 0]).  Eligible: stamp < below.  The eligible
    rows in the order (stamp ascending, row ascending); the first n of them; as global rows in ascending row order; -1 behind them."""
    stamps = np.asarray(stamps, dtype=np.int64)
    order = np.lexsort((np.arange(stamps.size), stamps))                # the last key is the primary one; stable
    order = order[stamps[order] < below]
    chosen = np.sort(order[:n])
    out = np.full(n, -1, dtype=np.int64)
    out[:chosen.size] = row_base + chosen
    return out, [int(chosen.size), int(order.size), int(stamps[chosen].max()) if chosen.size else U64_NONE, 0]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from emdr2_amd import _native
    import os
    if not os.path.exists(_native.LIB_PATH):
        g.build()
    return _native.lib()


def test_reference_with_uniform_stamps_is_the_row_order():
    for n_rows, n, base in ((1000, 64, 0), (300, 300, 7000), (5, 0, 3)):
        out, info = oldest_rows_reference(np.full(n_rows, 3), n, 4, base)
        assert np.array_equal(out, base + np.arange(n)) and info == [n, n_rows, 3 if n else U64_NONE, 0]
        out, info = oldest_rows_reference(np.full(n_rows, 3), n, 3, base)    # nobody is older than the weights
        assert (out == -1).all() and info == [0, 0, U64_NONE, 0]


@pytest.mark.parametrize("seed", range(6))
def test_reference_selects_the_oldest_and_breaks_ties_by_row(seed):
    rng = np.random.default_rng(seed)
    n_rows = int(rng.integers(50, 400))
    stamps = rng.integers(0, (4, 50, 1 << 31)[seed % 3], size=n_rows)
    below = int(np.sort(stamps)[int(rng.integers(1, n_rows))]) + int(rng.integers(0, 2))
    n = int(rng.integers(1, n_rows + 1))
    base = int(rng.integers(0, 1 << 40))
    out, info = oldest_rows_reference(stamps, n, below, base)
    eligible = np.nonzero(stamps < below)[0]
    k = min(n, eligible.size)
    assert info[:2] == [k, eligible.size] and info[3] == 0
    chosen = out[:k] - base
    assert (out[k:] == -1).all() and (np.diff(chosen) > 0).all() and np.isin(chosen, eligible).all()
    if k == 0:
        assert info[2] == U64_NONE
        return
    rest = np.setdiff1d(eligible, chosen)
    cut = int(stamps[chosen].max())
    assert info[2] == cut
    if rest.size:
        assert cut <= stamps[rest].min()                                 # every selected stamp <= every unselected eligible stamp
        tied_in, tied_out = chosen[stamps[chosen] == cut], rest[stamps[rest] == cut]
        if tied_out.size:
            assert tied_in.max() < tied_out.min()                        # among stamps equal to the cut: the lowest-numbered rows


def test_c_entries_validate_their_arguments_without_a_gpu(lib):
    """bad sizes, null and misaligned pointers come back as status codes before any launch"""
    n = ctypes.c_size_t()
    assert lib.emdr2_mips_oldest_rows_workspace_bytes(21015324, ctypes.byref(n)) == 0 and 0 < n.value < (1 << 20)
    full = n.value
    assert lib.emdr2_mips_oldest_rows_workspace_bytes(0, ctypes.byref(n)) == 0 and 0 < n.value <= full
    assert lib.emdr2_mips_oldest_rows_workspace_bytes(-1, ctypes.byref(n)) == -1
    assert lib.emdr2_mips_oldest_rows_workspace_bytes(1000, None) == -1
    p, off4 = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    call = lib.emdr2_mips_oldest_rows
    big = 1 << 30
    assert call(p, 1000, 0, 7, 64, p, None, p, big, None) == -1              # null out_info
    assert call(p, 1000, 0, 7, 64, p, p, None, big, None) == -1              # null workspace
    assert call(None, 1000, 0, 7, 64, p, p, p, big, None) == -1              # null stamps with rows to read
    assert call(p, 1000, 0, 7, 64, None, p, p, big, None) == -1              # null out_rows with rows wanted
    assert call(p, 1000, 0, 7, 1001, p, p, p, big, None) == -1               # n_want > n_rows
    assert call(p, 1000, 0, 7, -1, p, p, p, big, None) == -1
    assert call(p, -1, 0, 7, 0, p, p, p, big, None) == -1
    assert call(p, 1000, -1, 7, 64, p, p, p, big, None) == -1                # row_base < 0
    assert call(p, 1000, 0, 7, 64, p, off4, p, big, None) == -1              # out_info is 8-byte aligned
    assert call(p, 1000, 0, 7, 64, off4, p, p, big, None) == -1              # so is out_rows
    assert call(p, 1000, 0, 7, 64, p, p, off4, big, None) == -1              # the workspace: 16 bytes
    assert call(ctypes.c_void_p(4098), 1000, 0, 7, 64, p, p, p, big, None) == -1
    assert call(p, 1000, 0, 7, 64, p, p, p, full - 1, None) == -2            # workspace too small
    assert call(p, 1000, 0, 7, 64, p, p, p, 0, None) == -2


def test_the_flag_and_its_rules():
    from emdr2_amd import arguments
    assert arguments.parse_args(BASE).index_refresh_oldest_first is False
    args = arguments.parse_args(BASE + ["--index-refresh-oldest-first", "--async-indexer", "--index-refresh-in-place"])
    assert args.index_refresh_oldest_first is True and args.index_generations is True and args.index_newest_wins is False
    args = arguments.parse_args(BASE + ["--index-refresh-oldest-first", "--async-indexer", "--index-refresh-in-place", "--index-newest-wins",
                                        "--index-writeback", "--disable-retriever-dropout"])
    assert args.index_refresh_oldest_first and args.index_newest_wins and args.index_generations
    for missing in ([], ["--async-indexer"], ["--index-refresh-in-place"], ["--index-generations", "--async-indexer"]):
        with pytest.raises(ValueError, match="rolling refresher"):
            arguments.parse_args(BASE + ["--index-refresh-oldest-first"] + missing)
    help_text = " ".join(arguments.get_parser().format_help().split())
    for phrase in ("--index-refresh-oldest-first", "implies --index-generations", "OLDEST rows", "uniform stamps"):
        assert phrase in help_text, phrase


# -- the refresher's bookkeeping on a stub index ------------------------------------------------------------------------------------------
class _StampedStub(object):
    """an index of n rows from `row_base` on that keeps stamps on the host: `oldest_rows` is the numpy reference, `update_rows_at` the
    stamp rule; records every selection and every write"""
    generations = True

    def __init__(self, n, row_base=0, stamps=None):
        self.n, self.row_base = n, row_base
        self.stamps = np.zeros(n, dtype=np.int64) if stamps is None else np.array(stamps, dtype=np.int64)
        self.shard = type("Shard", (), {"ids": None, "dim": 8})()
        self.selections, self.writes, self.kept = [], [], 0

    def local_rows(self):
        return self.row_base, self.row_base + self.n

    def oldest_rows(self, n, below):
        out, info = oldest_rows_reference(self.stamps, min(n, self.n), below, self.row_base)
        self.selections.append((n, below))
        return torch.from_numpy(out), torch.tensor([w if w != U64_NONE else -1 for w in info], dtype=torch.int64)

    def update_rows_at(self, rows, embeds, generation=None, newest_wins=False):
        assert rows.shape[0] == embeds.shape[0]
        local = rows.numpy() - self.row_base
        local = local[(local >= 0) & (local < self.n)]
        newer = self.stamps[local] > generation if newest_wins else np.zeros(local.size, dtype=bool)
        self.kept += int(newer.sum())
        self.stamps[local[~newer]] = generation
        self.writes.append((local[~newer].tolist(), generation))


def test_oldest_first_needs_the_rolling_mode_and_stamps(monkeypatch):
    with pytest.raises(ValueError, match="oldest_first"):
        _builder(monkeypatch, _StampedStub(20), in_place=False, oldest_first=True)
    plain = _StampedStub(20)
    plain.generations = False
    with pytest.raises(ValueError, match="oldest_first"):
        _builder(monkeypatch, plain, in_place=True, oldest_first=True)


def test_oldest_first_on_uniform_stamps_is_the_sequential_pass_and_ends_with_the_last_eligible_row(monkeypatch):
    index = _StampedStub(35, row_base=100)                               # batches of 10: 30 rows per pump, then 5 and 25 empty slots
    seen = []
    b = _builder(monkeypatch, index, in_place=True, batches_per_pump=3, iteration=4, newest_wins=True, oldest_first=True)
    b.log = seen.append
    assert b.pump() is False and index.selections == [(30, 4)]
    assert [tuple(q[1].shape) for q in b._queued] == [(30, 8)] and index.writes == []      # nothing enters the index before the boundary
    assert b.maybe_swap(5) is True                                       # (the interval condition alone, as in the sequential form)
    assert index.writes == [(list(range(30)), 4)] and b.passes == 0 and (b.rows_selected, b.rows_padded) == (30, 0)
    b.pump()
    assert [tuple(q[1].shape) for q in b._queued] == [(30, 8)]          # fixed shapes: the five rows left and 25 empty slots
    b.maybe_swap(6)
    assert index.writes[1] == (list(range(30, 35)), 4) and (index.stamps == 4).all()
    assert b.passes == 1 and (b.rows_selected, b.rows_padded) == (35, 25) and b.snapshot_generation == 4
    assert seen == ["oldest-first pass 1 complete at iteration 6: 35 rows embedded, 25 slots padded"]
    # the next pump takes the snapshot of the step count the last boundary told the builder
    b.pump()
    assert b.snapshot_generation == 6 and index.selections[-1] == (30, 6)
    assert index.kept == 0


def test_oldest_first_never_selects_a_row_the_write_back_has_stamped_since_the_snapshot(monkeypatch):
    stamps = np.zeros(40, dtype=np.int64)
    stamps[[3, 4, 25]] = 7                                               # written back from the weights of step 7
    stamps[30:] = 2                                                      # a newer cluster: comes after every 0
    index = _StampedStub(40, stamps=stamps)
    b = _builder(monkeypatch, index, in_place=True, batches_per_pump=2, iteration=7, newest_wins=True, oldest_first=True)
    b.log = lambda msg: None
    b.pump(); b.maybe_swap(8)
    assert index.writes[0] == ([r for r in range(22) if r not in (3, 4)], 7)        # the 20 oldest, lowest rows first
    index.stamps[[23, 24]] = 8                                           # this boundary's write-back: two rows the pass will now skip
    b.pump(); b.maybe_swap(9)
    assert index.writes[1] == ([22, 26, 27, 28, 29] + list(range(30, 40)), 7)       # what is left of the zeros, then the twos
    assert b.passes == 1 and index.kept == 0 and (index.stamps >= 7).all()
    assert (b.rows_selected, b.rows_padded) == (35, 5)


def test_a_pass_of_generation_zero_ends_at_its_first_boundary_and_forced_drain_runs_until_a_pass_ends(monkeypatch):
    index = _StampedStub(25)
    b = _builder(monkeypatch, index, in_place=True, batches_per_pump=1, iteration=0, oldest_first=True)
    b.log = lambda msg: None
    b.pump(); b.maybe_swap(1)                                            # below = 0: nothing is eligible
    assert index.writes == [([], 0)] and b.passes == 1 and (b.rows_selected, b.rows_padded) == (0, 10)
    assert b.maybe_swap(9, force=True) is True                           # snapshot at 9; 10 + 10 + 5 rows
    assert [w[1] for w in index.writes[1:]] == [9, 9, 9] and sum(len(w[0]) for w in index.writes[1:]) == 25
    assert b.passes == 2 and (index.stamps == 9).all()
