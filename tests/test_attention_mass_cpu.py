"""CPU: the reader attention mass without a GPU.

  * tests/attention_mass_ref.py against a brute-force softmax on tiny inputs;
  * a torch fp32 model of csrc/attention_mass.hip's order of operations passes the bound, and planted defects in that model, one at a time,
    each exceed it (the `caught` table, as in test_gemm_ref_cpu);
  * the meter's arithmetic (tasks/openqa/e2eqa/reader_mass.py) on CPU tensors;
  * argument validation of emdr2_attention_key_mass through the library: the -1 and -4 cases of include/emdr2_ops.h;
  * the flag guards at the parser and at the model build."""
import ctypes
import math
import os

import pytest
import torch

from tests import attention_mass_ref as MR
from tests import attention_ref as R
from tests.test_context_from_index_cpu import BASE

L2E = 1.4426950408889634


def _tiny(seed=0, sq=5, sk=11, heads=2, hn=64, fam="randn"):
    g = torch.Generator().manual_seed(seed)
    q, k, _, _ = R.family(fam, 1, heads, sq, sk, hn, g)
    ids_q = torch.full((1, sq), 7, dtype=torch.int64)
    ids_k = torch.full((1, sk), 7, dtype=torch.int64)
    ids_q[0, 1] = 0
    ids_k[0, 3] = 0
    ids_k[0, sk - 2:] = 0
    seg = torch.tensor([[1, 4, 4, 9, sk - 1]], dtype=torch.int32)        # uncovered key 0 and sk - 1, an empty segment, masked keys inside
    w = torch.rand((1, sq), generator=g) + 0.25
    return q, k, ids_q, ids_k, seg, w


def _ref(q, k, ids_q, ids_k, seg, w, m=None, l=None):
    r = R.reference(q, k, torch.zeros_like(k), ids_q, ids_k, False)
    if m is None:
        m, l = MR.made_stats(r)
    return MR.mass_reference(q, list(k), ids_q, list(ids_k), m, l, seg, w) + (m, l)


@pytest.mark.parametrize("fam", ["randn", "one_hot"])
@pytest.mark.parametrize("weighted", [False, True])
def test_reference_against_brute_force_softmax(fam, weighted):
    q, k, ids_q, ids_k, seg, w = _tiny(3, fam=fam)
    w = w if weighted else None
    mass, bound, rows, _, _ = _ref(q, k, ids_q, ids_k, seg, w)
    brute = torch.tensor(MR.brute_force_mass(q[0], k[0], ids_q[0], ids_k[0], seg[0].tolist(), None if w is None else w[0]), dtype=torch.float64)
    # (m, l) are fp32 roundings of the float64 statistics: the two agree to that rounding, far inside the bound
    assert float((mass[0] - brute).abs().max()) <= 4 * 2.0 ** -24 * float(brute.abs().max())
    assert float(mass[0, :, 1].abs().max()) == 0.0                          # the empty segment
    assert bool((bound > 0).all())
    assert torch.allclose(rows[0], torch.ones_like(rows[0]), atol=1e-6)      # every row's probabilities sum to 1, padded queries' too


def model_mass(q, k, ids_q, ids_k, m, l, seg, w, fault=None):
    """The kernel's arithmetic in torch fp32 for ONE dense sequence batch: fp32 scores, x scale log2 e, the offset folded once per query,
    exp2, fp32 sums.  `fault`: one planted defect."""
    b, sq, n, d = q.shape
    sc2 = torch.tensor(L2E / math.sqrt(d), dtype=torch.float32)
    s2 = torch.einsum("bqnd,bknd->bnqk", q.float(), k.float()) * sc2
    masked = (ids_k == 0)[:, None, None, :].expand_as(s2)
    if fault != "masked_key_counted":
        s2 = torch.where(masked, torch.tensor(R.MASK_VALUE * L2E, dtype=torch.float32), s2)
    mm, ll = (m, l) if fault != "neighbour_head_stats" else (m.roll(1, dims=1), l.roll(1, dims=1))
    off2 = mm * torch.tensor(L2E, dtype=torch.float32) + (torch.log2(ll) if fault != "l_dropped" else 0.0)
    p = torch.exp2(s2 - off2[..., None])
    counted = torch.ones_like(ids_q, dtype=torch.float32) if fault == "pad_query_counted" else (ids_q != 0).float()
    wq = counted * (w.float() if (w is not None and fault != "weight_ignored") else 1.0)
    out = torch.zeros((b, n, seg.shape[1] - 1), dtype=torch.float32)
    for i in range(b):
        for g in range(seg.shape[1] - 1):
            lo, hi = int(seg[i, g]), int(seg[i, g + 1])
            if fault == "boundary_off_by_one":
                hi = min(hi + 1, k.shape[1]) if hi > lo else hi
            rows = p[i, :, :, lo:hi].sum(-1)                                         # (a select, like the kernel: a padded query's exp2 may be inf)
            out[i, :, g] = torch.where(wq[i][None] != 0, rows * wq[i][None], torch.zeros_like(rows)).sum(-1)
    return out


FAULTS = ("boundary_off_by_one", "l_dropped", "masked_key_counted", "neighbour_head_stats", "weight_ignored", "pad_query_counted")


def test_kernel_model_passes_and_planted_defects_are_caught():
    worst_ok, caught = 0.0, {f: False for f in FAULTS}
    for fam, seed in (("randn", 1), ("one_hot", 2), ("stair_up", 3)):
        q, k, ids_q, ids_k, seg, w = _tiny(seed, sq=7, sk=70, fam=fam)
        mass, bound, _, m, l = _ref(q, k, ids_q, ids_k, seg, w)
        ok = R.worst(model_mass(q, k, ids_q, ids_k, m, l, seg, w), mass, bound)[0]
        worst_ok = max(worst_ok, ok)
        for f in FAULTS:
            caught[f] = caught[f] or R.worst(model_mass(q, k, ids_q, ids_k, m, l, seg, w, fault=f), mass, bound)[0] > 1.0
    print("[mass-cpu] fp32 model worst err / bound %.3f; caught %s" % (worst_ok, caught))
    assert worst_ok < 1.0
    assert all(caught.values()), caught


def test_reduction_depth_is_the_kernels():
    assert MR.reduction_depth(1) == 4 + 18 and MR.reduction_depth(64) == 4 + 18 and MR.reduction_depth(65) == 8 + 18
    assert MR.reduction_depth(4200) == 4 * 66 + 18


# ---- the meter ------------------------------------------------------------------------------------------------------------------------
def test_normalise_mass_and_an_empty_question():
    from emdr2_amd.model.emdr2_model import normalise_mass
    x = torch.tensor([[1.0, 3.0, 0.0], [0.0, 0.0, 0.0], [2.0, 2.0, 4.0]])
    n = normalise_mass(x)
    assert torch.equal(n[1], torch.zeros(3)) and torch.allclose(n.sum(1), torch.tensor([1.0, 0.0, 1.0]))
    assert torch.allclose(n[0], torch.tensor([0.25, 0.75, 0.0]))


def test_meter_arithmetic_and_protocol():
    from emdr2_amd.tasks.openqa.e2eqa.reader_mass import ReaderMassMeter, mass_statistics
    mass = torch.tensor([[0.7, 0.2, 0.1], [0.0, 0.0, 0.0], [0.25, 0.5, 0.25], [1.0, 0.0, 0.0]])
    prior = torch.log_softmax(torch.tensor([[2.0, 1.0, 0.0], [0.0, 1.0, 2.0], [3.0, 1.0, 0.0], [0.0, 0.0, 5.0]]), dim=1)
    hits = torch.tensor([[False, True, False], [True, True, True], [False, True, True], [False, False, False]])
    want = MR.meter_reference(mass.tolist(), prior.tolist(), hits.tolist())
    got = dict(zip(("questions", "entropy", "agree", "hit_mass", "top1_hit"), mass_statistics(mass, prior, hits).tolist()))
    assert got["questions"] == want["questions"] == 3 and got["agree"] == want["agree"] == 1 and got["top1_hit"] == want["top1_hit"] == 1
    assert abs(got["entropy"] - want["entropy"]) < 1e-6 and abs(got["hit_mass"] - want["hit_mass"]) < 1e-6

    class Hits(object):                                        # what the meter reads of an AnswerHitTracker
        _step_hits = hits
    meter = ReaderMassMeter(3, Hits())
    meter.add(mass, prior, 0, 4)                               # not begun: a no-op (evaluation-mode forwards)
    meter.begin()
    meter.add(mass[:2], prior[:2], 0, 2)                       # a step that fails after its first group ...
    meter.begin()                                              # ... and is run again: counted once
    meter.add(mass[:2], prior[:2], 0, 2)
    meter.add(mass[2:], prior[2:], 2, 4)
    meter.commit()
    line = meter.line()
    assert line == " read entropy: {:.4f} | read-prior agree: 1/3 | read mass: {:.4f} | read top1 hit: 1/3 |".format(
        want["entropy"] / 3, want["hit_mass"] / 3), line
    assert meter.line() == " read entropy: 0.0000 | read-prior agree: 0/0 | read mass: 0.0000 | read top1 hit: 0/0 |"
    plain = ReaderMassMeter(3)
    plain.begin()
    plain.add(mass, prior, 0, 4)
    plain.commit()
    assert plain.line() == " read entropy: {:.4f} | read-prior agree: 1/3 |".format(want["entropy"] / 3)


# ---- the entry point's argument validation ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from emdr2_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        g.build()
    return _native.lib()


def _call(lib, **over):
    one = ctypes.c_void_p(4096)
    a = dict(q=one, q_sb=2048, q_ss=64, q_sn=64, k=one, k_sb=4096, k_ss=64, k_sn=64, ids_q=one, ids_k=one, cu_k=None, m=one, l=one, seg=one,
             w=None, mass=one, batch=1, heads=1, sq=32, max_sk=64, n_seg=2, head_dim=64, scale=0.125, accumulate=0, stream=None)
    a.update(over)
    return lib.emdr2_attention_key_mass(*[a[n] for n in ("q", "q_sb", "q_ss", "q_sn", "k", "k_sb", "k_ss", "k_sn", "ids_q", "ids_k", "cu_k", "m", "l",
                                                         "seg", "w", "mass", "batch", "heads", "sq", "max_sk", "n_seg", "head_dim", "scale",
                                                         "accumulate", "stream")])


def test_key_mass_entry_validates_its_arguments_without_a_gpu(lib):
    for name in ("q", "k", "ids_q", "ids_k", "m", "l", "seg", "mass"):
        assert _call(lib, **{name: None}) == -1, name
    for name in ("batch", "heads", "sq", "n_seg"):
        assert _call(lib, **{name: 0}) == -1, name
    assert _call(lib, q=ctypes.c_void_p(4096 + 8)) == -1 and _call(lib, k=ctypes.c_void_p(4096 + 2)) == -1      # misaligned bf16 operands
    assert _call(lib, head_dim=32) == -4
    assert _call(lib, sq=129) == -4
    assert _call(lib, max_sk=65537, cu_k=ctypes.c_void_p(4096)) == -4
    assert _call(lib, max_sk=48) == -4                                                                            # dense keys: whole 32-key steps
    assert _call(lib, k_ss=60) == -4


# ---- the flag guards --------------------------------------------------------------------------------------------------------------------------
def test_flag_parses_and_is_off_by_default():
    from emdr2_amd import arguments
    assert arguments.parse_args(BASE).reader_attention_mass is False
    assert arguments.parse_args(BASE + ["--reader-attention-mass"]).reader_attention_mass is True
    assert "--reader-attention-mass" in arguments.get_parser().format_help()


def test_flag_is_refused_with_other_head_sizes_and_with_fp32_validation():
    from emdr2_amd import arguments
    from emdr2_amd.model.emdr2_model import EMDR2Model, check_reader_attention_mass
    from emdr2_amd.model.transformer import Config
    with pytest.raises(ValueError, match="reader-attention-mass"):
        arguments.parse_args(BASE + ["--reader-attention-mass", "--fp32-validation"])
    narrow = [a for a in BASE]
    narrow[narrow.index("--kv-channels") + 1] = "32"
    narrow[narrow.index("--num-attention-heads") + 1] = "24"
    with pytest.raises(ValueError, match="reader-attention-mass"):
        arguments.parse_args(narrow + ["--reader-attention-mass"])
    check_reader_attention_mass(Config(hidden_size=128, num_attention_heads=2))
    with pytest.raises(ValueError, match="64 channels"):
        check_reader_attention_mass(Config(hidden_size=128, num_attention_heads=4))
    with pytest.raises(ValueError, match="fp32"):
        check_reader_attention_mass(Config(hidden_size=128, num_attention_heads=2, compute_dtype="fp32"))
    # the model build itself: refused before any module is made
    with pytest.raises(ValueError, match="64 channels"):
        EMDR2Model(None, Config(hidden_size=128, num_attention_heads=4), 512, 512, topk=3, seq_length=64, seq_length_ret=32, cls_id=1, sep_id=2,
                   reader_attention_mass=True)
