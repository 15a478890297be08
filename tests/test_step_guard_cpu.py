"""No GPU: the step guard (--skip-nonfinite-steps).  The numpy statements of the census and of the guard's state (tests/step_guard_ref.py;
the GPU tests compare the device with them), the two flags and their rules, the entry points' argument checks, FlatAdam's report and
checkpoint handling on host-built tables, and the interval-average rule of the training log."""
import ctypes

import numpy as np
import pytest
import torch

from tests import step_guard_ref as G

BASE = ("--task OPENQA --num-layers 2 --hidden-size 128 --num-attention-heads 2 --max-position-embeddings 64 --seq-length 64 "
        "--decoder-seq-length 32 --batch-size 4 --lr 2e-4").split()


def test_census_restatement_counts_and_keys():
    g = np.ones(10, dtype=np.float32)
    assert G.census(g) == [0, 0, G.NO_KEY, 0]
    g[7] = np.nan; g[3] = -np.inf; g[9] = np.inf
    assert G.census(g) == [1, 2, 3, 0]
    assert G.census(g, bucket=2) == [1, 2, (2 << 40) | 3, 0]
    # buckets merge: counts add, the smaller key wins whichever bucket came first
    assert G.census(g, bucket=1, prior=G.census(g, bucket=2)) == [2, 4, (1 << 40) | 3, 0]
    assert G.census(np.ones(4, np.float32), bucket=0, prior=G.census(g, bucket=2)) == [1, 2, (2 << 40) | 3, 0]
    # finite elements whose squares overflow are not the census's business
    assert G.census(np.full(2, 3e19, np.float32)) == [0, 0, G.NO_KEY, 0]


def test_state_restatement_runs_and_sticky_record():
    s = [0] * 8
    inf = np.float32(np.inf)
    seq = [(1.0, G.CENSUS_EMPTY), (np.nan, [1, 0, 5, 0]), (inf, [0, 2, (1 << 40) | 9, 0]), (2.0, G.CENSUS_EMPTY), (inf, G.CENSUS_EMPTY)]
    for step, (gsq, c) in enumerate(seq, start=1):
        s, left = G.verdict(gsq, c, s, step)
        assert left == G.CENSUS_EMPTY
    assert s[:4] == [1, 3, 1, 2]                                         # last skipped, three in total, run 1, longest 2
    assert s[4:] == [2, 5, 1, 0]                                         # the FIRST skip's record stays
    s[4:] = [0, 0, 0, 0]                                                 # cleared: the next skip refills it -- here an overflow over finite elements
    with np.errstate(over="ignore"):
        overflowed = np.float32(3e19) * np.float32(3e19)
    s, _ = G.verdict(overflowed, G.CENSUS_EMPTY, s, 6)
    assert s == [1, 4, 2, 2, 6, G.NO_KEY, 0, 0]
    s, _ = G.verdict(0.0, G.CENSUS_EMPTY, s, 7)
    assert s[:4] == [0, 4, 0, 2] and s[4] == 6


def test_flags_and_their_rules():
    from emdr2_amd import arguments
    args = arguments.parse_args(BASE)
    assert args.skip_nonfinite_steps is False and args.max_consecutive_skipped_steps == 0        # off by default, no limit
    args = arguments.parse_args(BASE + ["--skip-nonfinite-steps"])
    assert args.skip_nonfinite_steps is True and args.max_consecutive_skipped_steps == 0
    args = arguments.parse_args(BASE + ["--skip-nonfinite-steps", "--max-consecutive-skipped-steps", "5", "--deterministic-gradients",
                                        "--question-micro-batches", "2"])
    assert args.skip_nonfinite_steps and args.max_consecutive_skipped_steps == 5 and args.deterministic_gradients
    assert args.question_micro_batches == 2
    with pytest.raises(ValueError, match="fp32-validation"):
        arguments.parse_args(BASE + ["--skip-nonfinite-steps", "--fp32-validation"])
    with pytest.raises(ValueError):
        arguments.parse_args(BASE + ["--skip-nonfinite-steps", "--max-consecutive-skipped-steps", "-1"])
    with pytest.raises(ValueError, match="needs --skip-nonfinite-steps"):
        arguments.parse_args(BASE + ["--max-consecutive-skipped-steps", "3"])


def test_entry_points_are_bound_and_validate_their_arguments():
    """Null or misaligned pointers, empty shapes, a bucket number or a length the key cannot hold, step 0: refused (-1) before any launch."""
    from emdr2_amd import _native
    lib = _native.lib()
    al, off4 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 4)
    assert lib.emdr2_abi_version() == 4                                  # new entry points do not move it
    assert lib.emdr2_sumsq_census_f32(al, 8, al, al, None, 0, None) == -1
    assert lib.emdr2_sumsq_census_f32(None, 8, al, al, al, 0, None) == -1
    assert lib.emdr2_sumsq_census_f32(al, 0, al, al, al, 0, None) == -1
    assert lib.emdr2_sumsq_census_f32(al, 8, al, al, off4, 0, None) == -1
    assert lib.emdr2_sumsq_census_f32(al, 8, al, al, al, -1, None) == -1
    assert lib.emdr2_sumsq_census_f32(al, 8, al, al, al, 1 << 23, None) == -1
    assert lib.emdr2_sumsq_census_f32(al, 1 << 40, al, al, al, 0, None) == -1
    assert lib.emdr2_step_verdict(None, al, al, 1, None) == -1
    assert lib.emdr2_step_verdict(al, None, al, 1, None) == -1
    assert lib.emdr2_step_verdict(al, al, None, 1, None) == -1
    assert lib.emdr2_step_verdict(al, al, off4, 1, None) == -1
    assert lib.emdr2_step_verdict(al, al, al, 0, None) == -1
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0)
    assert lib.emdr2_adam_step_flat_guarded(al, al, al, al, al, 1028, 0, *hyper, 1, None, 0.0, None, None) == -1        # no state
    assert lib.emdr2_adam_step_flat_guarded(al, al, al, al, al, 1028, 0, *hyper, 1, None, 0.0, off4, None) == -1
    assert lib.emdr2_adam_step_flat_guarded(al, al, al, al, al, 1027, 0, *hyper, 1, None, 0.0, al, None) == -1          # the plain entry's rules
    assert lib.emdr2_adam_step_flat_guarded(al, al, al, al, al, 1028, 6, *hyper, 1, None, 0.0, al, None) == -1
    assert lib.emdr2_adam_step_flat_guarded(al, al, al, al, al, 1028, 0, *hyper, 0, None, 0.0, al, None) == -1


def _host_optimizer():
    from emdr2_amd.training import FlatAdam
    names, shapes = ["emb", "w1", "b1", "w2", "layernorm_weight", "w3"], [(50, 16), (64, 16), (61,), (16, 64), (3,), (300, 300)]
    mod = torch.nn.Module()
    for n, s_ in zip(names, shapes):
        mod.register_parameter(n, torch.nn.Parameter(torch.zeros(s_)))
    # host tensors: the layout and the bookkeeping only (small buckets: several of them)
    return mod, FlatAdam(mod, bucket_bytes=64 * 16 * 4 + 300, exchange_dtype="fp32")


def test_guard_on_host_tensors_raises_like_step():
    from emdr2_amd import _native
    from emdr2_amd.training import FlatAdam
    mod, opt = _host_optimizer()
    assert opt.skip_nonfinite is False
    with pytest.raises(_native.NativeError):
        opt.step()
    with pytest.raises(_native.NativeError):
        FlatAdam(mod, exchange_dtype="fp32", skip_nonfinite=True)
    with pytest.raises(RuntimeError):
        opt.guard_report()                                               # nothing to report with the guard off


def test_report_resolves_the_first_offender_on_a_host_built_slot_table():
    mod, opt = _host_optimizer()
    assert len(opt.buckets) >= 3
    named = dict(mod.named_parameters())
    for name, p in named.items():
        b, o, n = opt.slot[p]
        for e in (0, n // 2, n - 1):                                     # first, middle and last element of every tensor
            assert opt.resolve_offender((b["idx"] << 40) | (o + e)) == (name, e)
    b, o, n = opt.slot[named["b1"]]                                      # 61 elements in a slice of 64: the padding belongs to nobody
    assert opt.resolve_offender((b["idx"] << 40) | (o + 61)) == (None, None)
    assert opt.resolve_offender(G.NO_KEY) == (None, None) and opt.resolve_offender(-1) == (None, None)       # (an int64 view of all ones)
    assert opt.resolve_offender(len(opt.buckets) << 40) == (None, None)
    b, o, n = opt.slot[named["w2"]]
    key = (b["idx"] << 40) | (o + 17)
    rep = opt.report_from_words([1, 3, 1, 2, 7, key, 4, 1])
    assert rep == {"skipped_total": 3, "consecutive": 1, "longest_run": 2, "step": 7, "parameter": "w2", "element": 17, "nan": 4, "inf": 1}
    rep = opt.report_from_words([1, 1, 1, 1, 2, -1, 0, 0])               # the sum overflowed over finite elements
    assert rep["step"] == 2 and rep["parameter"] is None and rep["element"] is None and rep["nan"] == 0 and rep["inf"] == 0
    rep = opt.report_from_words([0, 5, 0, 3, 0, 0, 0, 0])                # record cleared
    assert rep["skipped_total"] == 5 and rep["longest_run"] == 3 and rep["step"] is None and rep["parameter"] is None


def test_state_dict_round_trip_with_and_without_the_count():
    mod, opt = _host_optimizer()
    sd = opt.state_dict()
    assert set(sd) == {"step", "state"}                                  # guard off: the reference-pinned layout
    opt.load_state_dict(dict(sd, step=4, skipped_steps=9))               # a checkpoint of a guarded run loads into an unguarded one
    assert opt.step_count == 4 and set(opt.state_dict()) == {"step", "state"}
    # the guard's host-visible side on a host-built state (the constructor refuses host tensors: the kernels are the guard)
    opt.skip_nonfinite, opt._guard_state = True, torch.zeros(8, dtype=torch.int64)
    opt._guard_state[1] = 3
    sd = opt.state_dict()
    assert set(sd) == {"step", "state", "skipped_steps"} and sd["skipped_steps"] == 3 and isinstance(sd["skipped_steps"], int)
    mod2, opt2 = _host_optimizer()
    opt2.skip_nonfinite, opt2._guard_state = True, torch.full((8,), 7, dtype=torch.int64)
    opt2.load_state_dict(sd)
    assert opt2._guard_state.tolist() == [0, 3, 0, 0, 0, 0, 0, 0] and opt2.guard_report()["skipped_total"] == 3
    del sd["skipped_steps"]                                              # a checkpoint written with the guard off: 0
    opt2.load_state_dict(sd)
    assert opt2._guard_state.tolist() == [0] * 8
    assert bool(opt2.last_step_skipped) is False
    opt2._guard_state[0] = 1
    assert bool(opt2.last_step_skipped) is True and opt2.last_step_skipped.dtype == torch.bool


def test_interval_average_divides_by_the_applied_steps():
    from emdr2_amd.tasks.openqa.e2eqa.train_e2eqa import interval_average, skipped_step_line
    assert interval_average(12.0, 4, 0) == 3.0
    assert interval_average(12.0, 4, 1) == 4.0
    assert interval_average(0.0, 4, 4) == 0.0 and interval_average(5.0, 2, 3) == 5.0      # max(1, .): training.py:298-306
    line = skipped_step_line({"step": 3, "parameter": "w2", "element": 17, "nan": 4, "inf": 1}, 3)
    assert "iteration 3" in line and "w2[17]" in line and "NaN elements: 4" in line and "Inf elements: 1" in line
    assert "overflowed" in skipped_step_line({"step": 3, "parameter": None, "element": None, "nan": 0, "inf": 0}, 3)
