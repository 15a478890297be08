"""No GPU: the parameter statistics (--log-param-stats-interval).  The host-only plan entry against its numpy restatement
(tests/param_stats_ref.py) at the parameter lengths where the chunk rule changes, its prefix table and what it rejects; the argument
checks of emdr2_param_stats with fake aligned pointers; the restatement's own ordered sum against math.fsum; the pure grouping helper and
the log lines on a hand-made record set; the flags and their rules."""
import ctypes

import numpy as np
import pytest

from tests import param_stats_ref as R
from tests.test_step_guard_cpu import BASE

LENGTHS = [1, 7, 8, 9, 8191, 8192, 8193, 2 * 8192 + 5]


def _layout(lengths):
    """FlatAdam._close's rule: every tensor starts at the next multiple of 8 elements."""
    offsets, off = [], 0
    for length in lengths:
        offsets.append(off)
        off += (length + 7) // 8 * 8
    return offsets, off


def _plan(offsets, lengths, n, count_only=False):
    """The entry itself -> (status, items, first, n_items)."""
    from emdr2_amd import _native
    lib = _native.lib()
    offs, lens = np.array(offsets, dtype=np.int64), np.array(lengths, dtype=np.int64)
    first, count = np.full(len(offsets) + 1, -7, dtype=np.int64), ctypes.c_int64(-7)
    status = lib.emdr2_param_stats_plan(offs.ctypes.data, lens.ctypes.data, len(offsets), n, None, first.ctypes.data, ctypes.byref(count))
    if status or count_only:
        return status, None, first, count.value
    items = np.full((count.value, 2), -7, dtype=np.int64)
    status = lib.emdr2_param_stats_plan(offs.ctypes.data, lens.ctypes.data, len(offsets), n, items.ctypes.data, first.ctypes.data,
                                        ctypes.byref(count))
    return status, items, first, count.value


def test_plan_entry_equals_the_restatement_at_the_lengths_where_the_chunk_rule_changes():
    offsets, n = _layout(LENGTHS)
    status, items, first, n_items = _plan(offsets, LENGTHS, n)
    want_items, want_first = R.plan(offsets, LENGTHS, n)
    assert status == 0 and n_items == len(want_items) == 1 + 1 + 1 + 1 + 1 + 1 + 2 + 3
    assert np.array_equal(items, want_items) and np.array_equal(first, want_first)
    # the prefix table: parameter p owns items first[p] .. first[p + 1], they tile the parameter from its own start and nothing else
    assert first[0] == 0 and first[-1] == n_items and first.tolist() == [0, 1, 2, 3, 4, 5, 6, 8, 11]
    covered = np.zeros(n, dtype=np.int32)
    for p, (off, length) in enumerate(zip(offsets, LENGTHS)):
        mine = items[first[p]:first[p + 1]]
        assert mine[0, 0] == off and int(mine[:, 1].sum()) == length
        assert all(int(x) == R.CHUNK for x in mine[:-1, 1]) and 1 <= int(mine[-1, 1]) <= R.CHUNK
        assert np.array_equal(mine[1:, 0], mine[:-1, 0] + mine[:-1, 1])
        for start, ln in mine:
            covered[start:start + ln] += 1
    owned = np.zeros(n, dtype=np.int32)
    for off, length in zip(offsets, LENGTHS):
        owned[off:off + length] = 1
    assert np.array_equal(covered, owned)                                # the padding between two tensors belongs to no item
    assert (items[:, 0] % 8 == 0).all()                                  # every item starts 32-byte aligned
    # counting alone gives the same count and the same prefix table
    status, _, first2, n2 = _plan(offsets, LENGTHS, n, count_only=True)
    assert status == 0 and n2 == n_items and np.array_equal(first2, first)


def test_plan_entry_rejects_malformed_buckets():
    offsets, n = _layout(LENGTHS)
    assert _plan(offsets, LENGTHS, n)[0] == 0
    bad = list(offsets); bad[3] += 4
    assert _plan(bad, LENGTHS, n)[0] == -1                               # an unaligned offset
    bad = list(offsets); bad[5] = offsets[4] + 8184
    assert _plan(bad, LENGTHS, n)[0] == -1                               # overlap: parameter 4 holds 8191 elements from offsets[4]
    bad = list(offsets); bad[2], bad[3] = offsets[3], offsets[2]
    assert _plan(bad, LENGTHS, n)[0] == -1                               # offsets that do not ascend
    assert _plan(offsets, LENGTHS, n - 8)[0] == -1                       # the last parameter ends past n
    assert _plan(offsets, LENGTHS[:-1] + [LENGTHS[-1] + 8], n)[0] == -1
    assert _plan(offsets, [0] + LENGTHS[1:], n)[0] == -1                 # zero length
    assert _plan(offsets, LENGTHS, n + 4)[0] == -1                       # n % 8
    assert _plan([-8], [4], 8)[0] == -1
    R.plan(offsets, LENGTHS, n)                                          # the restatement rejects what the entry rejects
    for args in ((bad, LENGTHS, n), (offsets, [0] + LENGTHS[1:], n), (offsets, LENGTHS, n - 8)):
        with pytest.raises(ValueError):
            R.plan(*args)
    from emdr2_amd import _native
    lib = _native.lib()
    one, count = np.zeros(2, dtype=np.int64), ctypes.c_int64()
    lens = np.array([8], dtype=np.int64)
    assert lib.emdr2_param_stats_plan(None, lens.ctypes.data, 1, 8, None, one.ctypes.data, ctypes.byref(count)) == -1
    assert lib.emdr2_param_stats_plan(one.ctypes.data, lens.ctypes.data, 0, 8, None, one.ctypes.data, ctypes.byref(count)) == -1
    assert lib.emdr2_param_stats_plan(one.ctypes.data, lens.ctypes.data, 1, 8, None, None, ctypes.byref(count)) == -1
    assert lib.emdr2_param_stats_plan(one.ctypes.data, lens.ctypes.data, 1, 8, None, one.ctypes.data, None) == -1
    assert lib.emdr2_param_stats_plan(one.ctypes.data, lens.ctypes.data, 1, 8, None, one.ctypes.data, ctypes.byref(count)) == 0 and count.value == 1


def test_stats_entry_validates_its_arguments_before_any_launch():
    from emdr2_amd import _native
    lib = _native.lib()
    al, off8, off4 = ctypes.c_void_p(4096), ctypes.c_void_p(4096 + 8), ctypes.c_void_p(4096 + 4)
    assert lib.emdr2_abi_version() == 4                                  # new entry points do not move it
    #       master grad m  v   n     items n_items first n_params beta1 beta2 eps  step ws  out stream
    good = [al, al, al, al, 8192, al, 1, al, 1, 0.9, 0.999, 1e-8, 1, al, al, None]
    for i in (0, 1, 2, 3, 5, 7, 13, 14):                                 # a null pointer in every place
        args = list(good)
        args[i] = None
        assert lib.emdr2_param_stats(*args) == -1, i
    for i in (0, 1, 2, 3):                                               # fp32 arrays: 16 bytes
        args = list(good)
        args[i] = off8
        assert lib.emdr2_param_stats(*args) == -1, i
    for i in (5, 7, 13, 14):                                             # plan, workspace, table: 8 bytes
        args = list(good)
        args[i] = off4
        assert lib.emdr2_param_stats(*args) == -1, i
    for i, value in ((4, 0), (4, 4), (4, 8196), (4, -8), (6, 0), (6, -1), (8, 0), (8, 2), (12, -1)):     # n, n_items, n_params (> n_items), step
        args = list(good)
        args[i] = value
        assert lib.emdr2_param_stats(*args) == -1, (i, value)
    size = ctypes.c_size_t()
    for n_items in (1, 11, 2900):
        assert lib.emdr2_param_stats_ws_bytes(n_items, ctypes.byref(size)) == 0 and size.value == n_items * 64
    assert lib.emdr2_param_stats_ws_bytes(0, ctypes.byref(size)) == -1 and lib.emdr2_param_stats_ws_bytes(1, None) == -1


@pytest.mark.parametrize("n", LENGTHS + [5 * 8192 + 77])
def test_restated_order_agrees_with_fsum_and_is_an_order(n):
    """The restatement's ordered sum against math.fsum: n non-negative doubles added in any order err by less than n * 2^-53 relative.
    A rotated array -- another order of the same values -- stays inside the same bound."""
    rng = np.random.default_rng(n)
    x = (rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, size=n))).astype(np.float32)
    got, truth = float(R.ordered_sum_sq(x)), R.fsum_sq(x)
    assert abs(got - truth) <= n * 2.0 ** -53 * truth
    assert abs(float(R.ordered_sum_sq(np.roll(x, 3))) - truth) <= n * 2.0 ** -53 * truth
    w = R.words(x, x)
    assert w[0] == w[1] and w[7] == n and w[2] == 0 and w[5] == int((x == 0).sum()) and w[6] == 0
    assert np.uint32(w[3]).view(np.float32) == np.abs(x).max()


RECORDS = {
    "language_model.embedding.word_embeddings.weight": dict(n=10, grad_sq=4.0, weight_sq=9.0, direction_sq=10.0, grad_zeros=1, grad_nonfinite=0,
                                                            max_abs_grad=1.5, max_abs_weight=2.0),
    "language_model.encoder.layers.0.attention.dense.weight": dict(n=6, grad_sq=1.0, weight_sq=16.0, direction_sq=2.0, grad_zeros=0,
                                                                   grad_nonfinite=2, max_abs_grad=float("inf"), max_abs_weight=3.0),
    "language_model.encoder.layers.0.attention.dense.bias": dict(n=2, grad_sq=3.0, weight_sq=9.0, direction_sq=6.0, grad_zeros=2,
                                                                 grad_nonfinite=0, max_abs_grad=0.5, max_abs_weight=4.0),
    "language_model.encoder.layers.11.mlp.dense_h_to_4h.weight": dict(n=4, grad_sq=0.0, weight_sq=1.0, direction_sq=0.0, grad_zeros=4,
                                                                      grad_nonfinite=0, max_abs_grad=0.0, max_abs_weight=1.0),
    "language_model.embedding.position_embeddings.weight": dict(n=6, grad_sq=5.0, weight_sq=7.0, direction_sq=6.0, grad_zeros=0, grad_nonfinite=0,
                                                                max_abs_grad=2.5, max_abs_weight=0.5),
    "lm_head_bias": dict(n=3, grad_sq=0.25, weight_sq=0.0, direction_sq=3.0, grad_zeros=0, grad_nonfinite=0, max_abs_grad=0.5, max_abs_weight=0.0),
}


def _stats():
    params = {}
    for name, r in RECORDS.items():
        params[name] = dict(r, grad_norm=r["grad_sq"] ** 0.5, weight_norm=r["weight_sq"] ** 0.5, direction_rms=(r["direction_sq"] / r["n"]) ** 0.5,
                            active=r["grad_sq"] > 0)
    return {"step": 7, "grads_current": True, "lr_note": "", "params": params}


def test_group_param_stats_on_a_hand_made_record_set():
    from emdr2_amd.training import group_param_stats, param_stats_group
    assert param_stats_group("a.layers.3.b.weight") == "a.layers.3" and param_stats_group("a.layers.weight") == "a.layers"
    assert param_stats_group("x.y.z") == "x.y" and param_stats_group("lm_head_bias") == "lm_head_bias"
    stats = _stats()
    groups = group_param_stats(stats)
    assert list(groups) == ["language_model.embedding", "language_model.encoder.layers.0", "language_model.encoder.layers.11", "lm_head_bias"]
    assert group_param_stats(stats["params"]) == groups                  # the 'params' dict alone will do
    emb, l0, l11, head = groups.values()
    assert (emb["params"], emb["n"], emb["grad_sq"], emb["weight_sq"], emb["direction_sq"], emb["grad_zeros"]) == (2, 16, 9.0, 16.0, 16.0, 1)
    assert (emb["grad_norm"], emb["weight_norm"], emb["direction_rms"], emb["max_abs_grad"], emb["max_abs_weight"]) == (3.0, 4.0, 1.0, 2.5, 2.0)
    assert (l0["params"], l0["n"], l0["grad_norm"], l0["weight_norm"], l0["direction_rms"]) == (2, 8, 2.0, 5.0, 1.0)
    assert (l0["grad_zeros"], l0["grad_nonfinite"], l0["max_abs_grad"], l0["max_abs_weight"]) == (2, 2, float("inf"), 4.0)
    assert (l11["grad_norm"], l11["direction_rms"], l11["grad_zeros"]) == (0.0, 0.0, 4)
    assert (head["n"], head["grad_norm"], head["direction_rms"]) == (3, 0.5, 1.0)
    assert sum(g["n"] for g in groups.values()) == sum(r["n"] for r in RECORDS.values())


def test_log_lines_name_the_norms_the_clip_factor_and_both_rankings():
    from emdr2_amd.tasks.openqa.e2eqa.train_e2eqa import param_stats_lines
    lines = param_stats_lines(_stats(), 40, lr=0.5, clip=1.0)
    assert len(lines) == 1 + 4
    gsq = sum(r["grad_sq"] for r in RECORDS.values())                    # 13.25
    head = lines[0]
    assert "param stats at iteration 40 (step 7, gradients current)" in head
    assert "grad norm: %.6E" % gsq ** 0.5 in head and "params norm: %.6E" % 42.0 ** 0.5 in head and "num zeros: 7" in head and "non-finite: 2" in head
    assert "clip factor: %.6f" % (1.0 / (gsq ** 0.5 + 1.0e-6)) in head
    # lr * |d| / |w|: embedding 0.5 * sqrt(10) / 3, position 0.5 * sqrt(6 / 7), bias 0.5 * sqrt(6) / 3, dense 0.5 * sqrt(2) / 4, layer 11: 0;
    # the head bias has no weight norm to be compared with
    moved = head.split("largest lr*|d|/|w|: ")[1].split(" | ")[0]
    assert [x.split(" ")[0] for x in moved.split(", ")] == [
        "language_model.embedding.word_embeddings.weight", "language_model.embedding.position_embeddings.weight",
        "language_model.encoder.layers.0.attention.dense.bias", "language_model.encoder.layers.0.attention.dense.weight",
        "language_model.encoder.layers.11.mlp.dense_h_to_4h.weight"]
    assert moved.startswith("language_model.embedding.word_embeddings.weight %.3E" % (0.5 * 10.0 ** 0.5 / 3.0))
    share = head.split("largest share of grad norm^2: ")[1]
    assert share.startswith("language_model.embedding.position_embeddings.weight %.1f%%, language_model.embedding.word_embeddings.weight %.1f%%"
                            % (500.0 / gsq, 400.0 / gsq))
    assert len(share.split(", ")) == 5
    assert lines[2].startswith(" param stats group language_model.encoder.layers.0: 2 tensors, 8 elements | grad norm: 2.000000E+00 | "
                               "params norm: 5.000000E+00 | direction rms: 1.000000E+00")
    assert "clip factor: 1.000000" in param_stats_lines(_stats(), 40, lr=0.5, clip=0.0)[0]         # clipping off


def test_flags_and_their_rules():
    from emdr2_amd import arguments
    args = arguments.parse_args(BASE)
    assert args.log_param_stats_interval == 0 and args.param_stats_file is None            # off by default
    args = arguments.parse_args(BASE + ["--log-param-stats-interval", "100", "--param-stats-file", "stats.jsonl"])
    assert args.log_param_stats_interval == 100 and args.param_stats_file == "stats.jsonl"
    with pytest.raises(ValueError, match="log-param-stats-interval"):
        arguments.parse_args(BASE + ["--log-param-stats-interval", "-1"])
    with pytest.raises(ValueError, match="fp32-validation"):
        arguments.parse_args(BASE + ["--log-param-stats-interval", "2", "--fp32-validation"])
    with pytest.raises(ValueError, match="param-stats-file"):
        arguments.parse_args(BASE + ["--param-stats-file", "stats.jsonl"])


def test_host_tensors_are_refused():
    from emdr2_amd import _native
    from tests.test_step_guard_cpu import _host_optimizer
    _, opt = _host_optimizer()
    with pytest.raises(_native.NativeError, match="HIP kernels only"):
        opt.param_stats()
