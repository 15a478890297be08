"""No GPU: generation stamps of the evidence index.  The numpy statements of the newest-wins rule and of the statistics report that the
GPU tests compare the device with (tests/test_index_generations_gpu.py imports them), the argument validation of the three entry points,
the two flags' rules, and the generation bookkeeping of the asynchronous refresher on a stub index."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

GEN_WORDS = 37
U64_NONE = (1 << 64) - 1


# -- the rule (include/emdr2_mips.h: emdr2_mips_update_rows_stamped, _update_rows_scattered_stamped) -----------------------------------
def apply_range(m, stamps, lo, new, gen, newest_wins):
    """rows [lo, lo + len(new)) of the matrix `m` and of the stamp vector, in place -> rows kept newer"""
    kept = 0
    for i in range(new.shape[0]):
        r = lo + i
        if newest_wins and stamps[r] > gen:                              # non-strict: a tie writes
            kept += 1
            continue
        m[r] = new[i]
        stamps[r] = gen
    return kept


def apply_list(m, stamps, ids, new, gen, newest_wins):
    """a list update: ids outside [0, n) are skipped and never counted; of a row named several times the LAST occurrence is the one the
    rule is applied to -> rows kept newer"""
    last = {int(r): i for i, r in enumerate(ids) if 0 <= r < m.shape[0]}
    kept = 0
    for r, i in last.items():
        if newest_wins and stamps[r] > gen:
            kept += 1
            continue
        m[r] = new[i]
        stamps[r] = gen
    return kept


# -- the report (emdr2_mips_generation_stats) -------------------------------------------------------------------------------------------
def stats_words(stamps, now, row_base=0, global_rows=None):
    """the EMDR2_GEN_WORDS report words as Python ints"""
    stamps = np.asarray(stamps, dtype=np.int64)
    if global_rows is None:
        g = stamps
    else:
        rows = np.asarray(global_rows, dtype=np.int64).reshape(-1)
        rows = rows[(rows >= row_base) & (rows < row_base + stamps.shape[0])]
        g = stamps[rows - row_base]                                      # a row named twice counts twice
    age = np.where(g > now, 0, now - g)
    words = [int(g.shape[0]), int(age.sum()), int(age.min()) if g.shape[0] else U64_NONE, int(age.max()) if g.shape[0] else 0, int((g > now).sum())]
    hist = [0] * 32
    for a in age.tolist():
        hist[min(int(a).bit_length(), 31)] += 1                          # 0 -> bin 0; [2^(b-1), 2^b) -> bin b
    return words + hist


def test_the_numpy_rule_on_a_sequence_of_range_and_list_updates():
    rng = np.random.default_rng(0)
    n, dim = 40, 4
    m = rng.standard_normal((n, dim)).astype(np.float16)
    stamps = np.zeros(n, dtype=np.int64)
    fresh = lambda k: rng.standard_normal((k, dim)).astype(np.float16)
    # a write-back at generation 7 over rows 3, 5, 5 (the last 5 wins), an invalid id and one past the end
    new = fresh(5)
    assert apply_list(m, stamps, [3, 5, -1, 5, n], new, 7, True) == 0
    assert stamps[3] == stamps[5] == 7 and np.array_equal(m[5], new[3]) and np.array_equal(m[3], new[0]) and stamps.sum() == 14
    # the refresher's pass of generation 4 comes round: rows 3 and 5 are newer and stay, every other row of the range is stamped 4
    before = m.copy()
    new = fresh(8)
    assert apply_range(m, stamps, 0, new, 4, True) == 2
    assert np.array_equal(m[[3, 5]], before[[3, 5]]) and stamps[:8].tolist() == [4, 4, 4, 7, 4, 7, 4, 4]
    assert np.array_equal(m[[0, 1, 2, 4, 6, 7]], new[[0, 1, 2, 4, 6, 7]])
    # a tie writes: two writers of one generation keep "the last one wins"
    new = fresh(1)
    assert apply_range(m, stamps, 3, new, 7, True) == 0 and np.array_equal(m[3], new[0]) and stamps[3] == 7
    # without newest-wins everything is overwritten and re-stamped, also downwards
    new = fresh(8)
    assert apply_range(m, stamps, 0, new, 2, False) == 0 and stamps[:8].tolist() == [2] * 8 and np.array_equal(m[:8], new)
    # a list whose rows are all newer changes nothing and counts each row once, however often it is named
    before, sb = m.copy(), stamps.copy()
    assert apply_list(m, stamps, [0, 1, 1, 0, 2], fresh(5), 1, True) == 3
    assert np.array_equal(m, before) and np.array_equal(stamps, sb)
    assert apply_list(m, stamps, [], fresh(0), 9, True) == 0


def test_the_numpy_report():
    stamps = [0, 5, 9, 10, 12, 3]
    w = stats_words(stamps, 10)
    ages = [10, 5, 1, 0, 0, 7]                                           # the stamp 12 lies beyond `now`: age 0, counted in word 4
    assert w[:5] == [6, sum(ages), 0, 10, 1]
    hist = w[5:]
    assert len(w) == GEN_WORDS and sum(hist) == 6
    assert hist[0] == 2 and hist[1] == 1 and hist[3] == 2 and hist[4] == 1     # 0, 0 | 1 | 5, 7 in [4, 8) | 10 in [8, 16)
    # a hit list: rows of other shards and negative entries are left out, a row named twice counts twice
    w = stats_words(stamps, 10, row_base=100, global_rows=[[101, 101, 99], [-1, 106, 105]])
    assert w[:5] == [3, 5 + 5 + 7, 5, 7, 0] and w[5 + 3] == 3
    assert stats_words(stamps, 10, row_base=100, global_rows=[])[:5] == [0, 0, U64_NONE, 0, 0]
    assert stats_words([], 10)[:5] == [0, 0, U64_NONE, 0, 0]
    assert stats_words([0], (1 << 31) - 1)[5 + 31] == 1                  # the largest age stamps below 2^31 can give


# -- argument validation of the entry points, before any launch -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from emdr2_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        g.build()
    return _native.lib()


def test_stamped_entry_points_reject_bad_arguments_before_any_launch(lib):
    from emdr2_amd import _native
    assert _native.GEN_WORDS == GEN_WORDS and len(_native.GEN_NAMES) == 5
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
    big = 1 << 20
    rng_call = lib.emdr2_mips_update_rows_stamped
    assert rng_call(p, 10, 768, 0, 1000, p, p, p, None, None, None, None, 5, 1, None, None) == -1       # no stamp array
    assert rng_call(p, 10, 768, 0, 1000, p, p, p, None, None, None, odd, 5, 1, None, None) == -1        # misaligned stamp array
    assert rng_call(p, 10, 768, 0, 1000, p, p, p, None, None, None, p, 5, 1, odd, None) == -1           # misaligned counter
    assert rng_call(p, 10, 768, 0, 1000, p, p, p, None, None, None, p, 1 << 31, 1, None, None) == -1    # generations are below 2^31
    assert rng_call(None, 10, 768, 0, 1000, p, p, p, None, None, None, p, 5, 1, None, None) == -1       # the unstamped form's own checks
    assert rng_call(p, 10, 768, 995, 1000, p, p, p, None, None, None, p, 5, 1, None, None) == -1
    assert rng_call(p, 0, 768, 0, 1000, p, p, p, None, None, None, p, 5, 1, None, None) == 0            # nothing to do launches nothing
    lst_call = lib.emdr2_mips_update_rows_scattered_stamped
    assert lst_call(p, p, 10, 768, 1000, p, p, p, None, None, None, p, big, None, 5, 0, None, None) == -1
    assert lst_call(p, p, 10, 768, 1000, p, p, p, None, None, None, p, big, p, 1 << 31, 0, None, None) == -1
    assert lst_call(p, None, 10, 768, 1000, p, p, p, None, None, None, p, big, p, 5, 0, None, None) == -1
    assert lst_call(p, p, 10, 768, 1000, p, p, p, None, None, None, p, 16, p, 5, 0, None, None) == -2    # workspace too small
    assert lst_call(p, p, 0, 768, 1000, p, p, p, None, None, None, p, big, p, 5, 0, None, None) == 0
    stats = lib.emdr2_mips_generation_stats
    assert stats(p, 1000, 0, None, 0, 7, None, None) == -1                                             # no report
    assert stats(p, 1000, 0, None, 0, 7, ctypes.c_void_p(4100), None) == -1                            # report not 8-byte aligned
    assert stats(None, 1000, 0, None, 0, 7, p, None) == -1                                             # rows without stamps
    assert stats(p, -1, 0, None, 0, 7, p, None) == -1
    assert stats(p, 1000, -1, None, 0, 7, p, None) == -1
    assert stats(p, 1000, 0, p, -1, 7, p, None) == -1


# -- the flags --------------------------------------------------------------------------------------------------------------------------
BASE = ("--task OPENQA --num-layers 2 --hidden-size 128 --num-attention-heads 2 --max-position-embeddings 64 --seq-length 64 "
        "--decoder-seq-length 32 --batch-size 4 --lr 2e-4").split()


def test_generation_flags_and_their_rules():
    from emdr2_amd import arguments
    args = arguments.parse_args(BASE)
    assert args.index_generations is False and args.index_newest_wins is False           # both off by default
    args = arguments.parse_args(BASE + ["--index-generations"])
    assert args.index_generations is True and args.index_newest_wins is False            # stamps alone: every writer still overwrites
    # newest-wins needs an in-place writer and implies the stamps
    for writer in (["--index-writeback", "--disable-retriever-dropout"], ["--async-indexer", "--index-refresh-in-place"],
                   ["--index-writeback", "--disable-retriever-dropout", "--async-indexer", "--index-refresh-in-place"]):
        args = arguments.parse_args(BASE + ["--index-newest-wins"] + writer)
        assert args.index_newest_wins is True and args.index_generations is True
    for no_writer in ([], ["--async-indexer"], ["--index-refresh-in-place"], ["--index-generations"]):
        with pytest.raises(ValueError, match="in-place writer"):
            arguments.parse_args(BASE + ["--index-newest-wins"] + no_writer)
    help_text = " ".join(arguments.get_parser().format_help().split())
    for phrase in ("--index-generations", "--index-newest-wins", "from the NEWEST weights", "semantics, not a tuning knob", "Ties write",
                   "unless --index-newest-wins is given"):
        assert phrase in help_text, phrase


# -- the refresher's bookkeeping on a stub index ----------------------------------------------------------------------------------------
class _StubIndex(object):
    """records (first, n, generation, newest_wins) of every in-place update and the generation of every swap pass"""
    generations = True

    def __init__(self, n):
        self.n, self.updates, self.passes, self.refreshed, self.commits = n, [], [], 0, 0
        self.shard = type("Shard", (), {"ids": None})()

    def local_rows(self):
        return 0, self.n

    def update_rows(self, first, rows, generation=None, newest_wins=False):
        self.updates.append((first, rows.shape[0], generation, newest_wins))

    def begin_refresh(self, generation=0):
        self.passes.append(generation)

    def refresh_rows(self, first, rows):
        self.refreshed += rows.shape[0]

    def commit_refresh(self):
        self.commits += 1


class _FakeStream(object):
    def wait_stream(self, other): pass
    def wait_event(self, event): pass
    def synchronize(self): pass


class _FakeEvent(object):
    def __init__(self, *a, **k): pass
    def record(self, stream=None): pass
    def query(self): return True


def _builder(monkeypatch, index, **kw):
    """an AsyncIndexBuilder over `index` whose side stream, events and encoder are stand-ins: everything else is the real code"""
    from emdr2_amd.tasks.openqa.e2eqa.async_indexer import AsyncIndexBuilder
    monkeypatch.setattr(torch.cuda, "Stream", _FakeStream)
    monkeypatch.setattr(torch.cuda, "Event", _FakeEvent)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: _FakeStream())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, s: None)
    monkeypatch.setattr(AsyncIndexBuilder, "embed", lambda self, doc_ids: torch.zeros((len(doc_ids), 8), dtype=torch.float16))
    return AsyncIndexBuilder(torch.nn.Linear(2, 2), None, index, 32, 1, 2, batch_size=10, index_reload_interval=4, **kw)


def test_rolling_refresher_queues_the_generation_of_the_pass_that_embedded_each_batch(monkeypatch):
    index = _StubIndex(35)                                               # four batches of 10, 10, 10, 5 rows
    b = _builder(monkeypatch, index, in_place=True, batches_per_pump=3, iteration=100, newest_wins=True)
    assert b.snapshot_generation == 100 and b.stamped and b.newest_wins
    # step 101: three batches of the first pass
    assert b.pump() is False
    b.maybe_swap(101)
    assert index.updates == [(0, 30, 100, True)]
    # step 102: the pass ends inside this pump after one batch; the next snapshot is taken with 101 steps complete -- the count the previous
    # boundary told the builder -- while the batch of the old pass is still in the queue with ITS generation
    assert b.pump() is True
    assert b.snapshot_generation == 101 and b.passes == 1
    assert [q[0] for q in b._queued] == [30] and [q[3] for q in b._queued] == [100]
    # a second pump before the boundary: batches of the new pass queue up behind it
    assert b.pump() is False
    assert [(q[0], q[1].shape[0], q[3]) for q in b._queued] == [(30, 5, 100), (0, 30, 101)]
    b.maybe_swap(102)
    assert index.updates[1:] == [(30, 5, 100, True), (0, 30, 101, True)]
    # a forced drain at a later boundary finishes the pass of generation 101 and snapshots at that boundary's count
    b.maybe_swap(110, force=True)
    assert index.updates[3:] == [(30, 5, 101, True)] and b.snapshot_generation == 110 and b.passes == 2


def test_rolling_refresher_on_an_unstamped_index_calls_update_rows_as_before(monkeypatch):
    index = _StubIndex(20)
    index.generations = False
    calls = []
    index.update_rows = lambda first, rows: calls.append((first, rows.shape[0]))          # takes no keywords: the old signature
    b = _builder(monkeypatch, index, in_place=True, batches_per_pump=1)
    b.pump(); b.maybe_swap(1); b.pump(); b.maybe_swap(2)
    assert calls == [(0, 10), (10, 10)]
    with pytest.raises(ValueError):
        _builder(monkeypatch, index, in_place=True, newest_wins=True)     # nothing to compare stamps with
    with pytest.raises(ValueError):
        _builder(monkeypatch, _StubIndex(20), in_place=False, newest_wins=True)   # the swap refresher replaces whole images


def test_swap_refresher_stamps_one_generation_per_pass(monkeypatch):
    index = _StubIndex(20)
    b = _builder(monkeypatch, index, in_place=False, batches_per_pump=1, iteration=7)
    assert b.pump() is False and index.passes == [7]                     # (begin_refresh runs with the pass's first batch)
    assert b.pump() is False and b.pump() is True
    assert b.maybe_swap(3) is False and b.steps_done == 3                # the reload interval (4) has not gone by; the count is remembered
    b.start()                                                            # (what maybe_swap does behind its commit, which needs a device)
    assert b.snapshot_generation == 3
    b.pump()
    assert index.passes == [7, 3]


def test_the_write_back_stamps_the_weights_the_forward_ran_with(monkeypatch):
    """`_train` hands `index_writeback` generation = `writeback_generation(iteration)` = iteration - 1 at the boundary after step
    `iteration`; an index without stamps gets the call it always got."""
    from emdr2_amd.tasks.openqa.e2eqa import train_e2eqa
    seen = []

    class Index(object):
        def update_rows_at(self, rows, embeds, **kw):
            seen.append((tuple(rows.shape), kw))

    class Retriever(object):
        mips_index, process_group = Index(), None

        def _world(self):
            return 0, 1

    class Model(object):
        evidence_retriever, hidden_size = Retriever(), 8

        def take_writeback(self):
            return None
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch, "device", lambda *a: "cpu")
    train_e2eqa.index_writeback(Model(), 2, 3)
    train_e2eqa.index_writeback(Model(), 2, 3, generation=41, newest_wins=True)
    assert seen == [((6,), {}), ((6,), {"generation": 41, "newest_wins": True})]
    assert [train_e2eqa.writeback_generation(i) for i in (1, 2, 500)] == [0, 1, 499]
