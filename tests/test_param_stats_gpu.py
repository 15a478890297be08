"""GPU: the parameter statistics.  emdr2_param_stats against its numpy restatement (tests/param_stats_ref.py) -- the float64 sums bit
for bit in the stated order, maxima and counts exactly -- on one bucket whose parameters have the lengths where the chunk rule and the
tail mask change, with NaN bit patterns in every padding element; planted zeros, denormals, infinities and NaNs; more items than the
capped grid has workgroups; step 0; FlatAdam.param_stats() after a real step on the two-layer T5Model of tests/test_dist_gpu.py against
torch float64 reductions; two data-parallel ranks whose tables are the same bits."""
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import param_stats_ref as R
from tests.test_dist_gpu import _init
from tests.test_param_stats_cpu import LENGTHS, _layout

pytestmark = pytest.mark.gpu
GRID_CAP = 1024                                                          # workgroups of the first launch (include/emdr2_ops.h)
NAN_BITS = (0x7fc00000, 0xffc00001, 0x7f800001, 0xffffffff)              # what the padding is filled with
BETA1, BETA2, EPS = 0.5, 0.75, 1e-8                                      # bias corrections exact in any arithmetic: 0.5, 0.875; 0.25, 0.578125


def _bucket(lengths, seed):
    """{'g', 'w', 'm', 'v'}: fp32 [n] with NaN patterns wherever no parameter lives, plus the layout."""
    offsets, n = _layout(lengths)
    rng = np.random.default_rng(seed)
    arrays = {}
    for k in "gwmv":
        arrays[k] = np.resize(np.array(NAN_BITS, dtype=np.uint32), n).view(np.float32).copy()
    for off, ln in zip(offsets, lengths):
        arrays["g"][off:off + ln] = (rng.standard_normal(ln) * np.exp(rng.uniform(-6, 2, size=ln))).astype(np.float32)
        arrays["w"][off:off + ln] = (rng.standard_normal(ln) * 0.05).astype(np.float32)
        arrays["m"][off:off + ln] = (rng.standard_normal(ln) * 1e-3).astype(np.float32)
        arrays["v"][off:off + ln] = (rng.standard_normal(ln) ** 2 * 1e-6).astype(np.float32)
    return arrays, offsets, n


def _device_stats(arrays, offsets, lengths, n, step, beta1=BETA1, beta2=BETA2, eps=EPS):
    """One call through the plan entry -> uint64 [n_params, 8] on the host.  The bucket is cloned before and compared after."""
    from emdr2_amd import _native
    from tests.test_param_stats_cpu import _plan
    lib = _native.lib()
    status, items, first, n_items = _plan(offsets, lengths, n)
    assert status == 0
    dev = {k: torch.from_numpy(arrays[k].view(np.int32)).cuda() for k in "gwmv"}
    before = {k: x.clone() for k, x in dev.items()}
    items_d, first_d = torch.from_numpy(items).cuda(), torch.from_numpy(first).cuda()
    ws = torch.full((n_items * R.WORDS,), 0x5555, dtype=torch.int64, device="cuda")
    out = torch.full((len(lengths), R.WORDS), 0x5555, dtype=torch.int64, device="cuda")          # (the call writes every word itself)
    _native.check(lib.emdr2_param_stats(dev["w"].data_ptr(), dev["g"].data_ptr(), dev["m"].data_ptr(), dev["v"].data_ptr(), n, items_d.data_ptr(),
                                        n_items, first_d.data_ptr(), len(lengths), beta1, beta2, eps, step, ws.data_ptr(), out.data_ptr(),
                                        _native.stream_ptr()), "param_stats")
    torch.cuda.synchronize()
    assert all(torch.equal(dev[k], before[k]) for k in "gwmv")           # it reads the bucket and writes nothing of it
    return out.cpu().numpy().view(np.uint64)


def _f64(word):
    return float(np.uint64(word).view(np.float64))


# ---- (a) the eight lengths in one bucket, NaN in every padding element ------------------------------------------------------------------
@pytest.fixture(scope="module")
def eight():
    arrays, offsets, n = _bucket(LENGTHS, seed=11)
    for off, ln in zip(offsets, LENGTHS):                                # the moments' special elements, in every parameter they fit in
        m, v = arrays["m"][off:off + ln], arrays["v"][off:off + ln]
        m[0], v[0] = 0.0, 0.0                                            # d = 0 / (0 + eps)
        if ln >= 9:
            v[ln // 2] = 1e-38                                           # below the smallest normal fp32
            m[ln - 1], v[ln - 1] = 3e4, 1e9
            m[3], v[3] = 0.0, 0.0
    want = [R.words(arrays["g"][o:o + ln], arrays["w"][o:o + ln]) for o, ln in zip(offsets, LENGTHS)]
    return arrays, offsets, n, want


@pytest.mark.parametrize("step", [1, 3])
def test_eight_lengths_in_one_bucket_equal_the_restatement_and_never_read_the_padding(eight, step):
    arrays, offsets, n, want = eight
    got = _device_stats(arrays, offsets, LENGTHS, n, step)
    for p, (off, ln) in enumerate(zip(offsets, LENGTHS)):
        row = [int(x) for x in got[p]]
        print("length %d step %d: device %s" % (ln, step, ["%#x" % x for x in row]))
        assert [row[i] for i in (0, 1, 3, 4, 5, 6, 7)] == [want[p][i] for i in (0, 1, 3, 4, 5, 6, 7)], ln     # bit for bit
        truth = R.fsum_sq(arrays["g"][off:off + ln])
        assert abs(_f64(row[0]) - truth) <= 1e-12 * truth, ln            # <= 2^15 non-negative doubles in any order: < 2^15 * 2^-53 ~ 4e-12 relative
        d = R.direction64(arrays["m"][off:off + ln], arrays["v"][off:off + ln], BETA1, BETA2, EPS, step)
        dsq = math.fsum(float(x) * float(x) for x in d)
        print("   sum d^2: device %.17g float64 %.17g relative %.3g" % (_f64(row[2]), dsq, abs(_f64(row[2]) - dsq) / dsq if dsq else 0.0))
        assert abs(_f64(row[2]) - dsq) <= 2e-6 * dsq, ln                 # four fp32 roundings in d, doubled by the square: <= 5e-7
        assert math.isfinite(_f64(row[2])) and (dsq > 0 or ln == 1)


# ---- (b) planted values ---------------------------------------------------------------------------------------------------------------------
def test_planted_zeros_denormals_infinities_and_nans_are_counted_and_the_nans_stay_out_of_the_maxima():
    lengths = [40, 2 * 8192 + 21, 24]
    arrays, offsets, n = _bucket(lengths, seed=5)
    off, ln = offsets[1], lengths[1]
    g, w = arrays["g"][off:off + ln].view(np.uint32), arrays["w"][off:off + ln].view(np.uint32)
    assert not ((g & 0x7fffffff) == 0).any()
    plants = {0: 0x00000000, 8191: 0x80000000, 8192: 0x00000001, 8193: 0x807fffff, 5: 0x7f800000, ln - 1: 0xff800000, 100: 0x7fc00000,
              2 * 8192 + 20 - 3: 0xffffffff, 16384: 0x80000000}
    for i, b in plants.items():
        g[i] = b
    w[7], w[9000] = 0x7fc12345, 0xffffffff                               # NaN weights: out of max |w|, and no business of the gradient's counts
    got = _device_stats(arrays, offsets, lengths, n, step=1)
    row = [int(x) for x in got[1]]
    want = R.words(arrays["g"][off:off + ln], arrays["w"][off:off + ln])
    assert row[5] == 3 and row[6] == 4                                   # +0, -0, -0; +Inf, -Inf and two NaNs; the denormals are neither
    assert row[3] == 0x7f800000                                          # max |g| is Inf, not a NaN pattern
    finite_w = arrays["w"][off:off + ln][~np.isnan(arrays["w"][off:off + ln])]
    assert np.uint32(row[4]).view(np.float32) == np.abs(finite_w).max()
    assert row[3:] == want[3:] and math.isnan(_f64(row[0])) and math.isnan(_f64(row[1]))
    for p in (0, 2):                                                     # the neighbours saw none of it
        rowp = [int(x) for x in got[p]]
        wantp = R.words(arrays["g"][offsets[p]:offsets[p] + lengths[p]], arrays["w"][offsets[p]:offsets[p] + lengths[p]])
        assert [rowp[i] for i in (0, 1, 3, 4, 5, 6, 7)] == [wantp[i] for i in (0, 1, 3, 4, 5, 6, 7)] and rowp[5] == 0 and rowp[6] == 0


# ---- (c) more items than workgroups --------------------------------------------------------------------------------------------------------
def test_more_items_than_workgroups_bit_for_bit():
    lengths = [(GRID_CAP + 1) * 8192 + 3]
    offsets, n = _layout(lengths)
    rng = np.random.default_rng(9)                                       # (fp32 draws: this bucket is 8.4 M elements)
    arrays = {k: np.resize(np.array(NAN_BITS, dtype=np.uint32), n).view(np.float32).copy() for k in "gwmv"}
    arrays["g"][:lengths[0]] = rng.standard_normal(lengths[0], dtype=np.float32) * np.float32(3.0)
    arrays["w"][:lengths[0]] = rng.standard_normal(lengths[0], dtype=np.float32) * np.float32(0.05)
    arrays["m"][:lengths[0]], arrays["v"][:lengths[0]] = 1e-3, 1e-6
    got = _device_stats(arrays, offsets, lengths, n, step=1)
    want = R.words(arrays["g"][:lengths[0]], arrays["w"][:lengths[0]])
    row = [int(x) for x in got[0]]
    assert row[0] == want[0] and row[1] == want[1]
    assert row[3:] == want[3:] and row[7] == lengths[0]


# ---- (d) step 0 -----------------------------------------------------------------------------------------------------------------------------
def test_step_zero_gives_a_zero_direction_and_does_not_read_the_moments(eight):
    arrays, offsets, n, want = eight
    poisoned = dict(arrays)
    for k in "mv":
        poisoned[k] = np.resize(np.array(NAN_BITS, dtype=np.uint32), n).view(np.float32).copy()
    got = _device_stats(poisoned, offsets, LENGTHS, n, step=0)
    for p in range(len(LENGTHS)):
        assert [int(x) for x in got[p]] == want[p]                       # word 2 of the restatement without d is 0


# ---- (e) FlatAdam.param_stats() ------------------------------------------------------------------------------------------------------------
def _build(seed=0):
    from emdr2_amd.model import kernels as K
    from emdr2_amd.model.transformer import Config, T5Model
    from emdr2_amd.training import FlatAdam
    torch.manual_seed(seed)
    cfg = Config(num_layers=2, hidden_size=128, num_attention_heads=2, ffn_hidden_size=256, max_position_embeddings=128, init_method_std=0.05)
    m = T5Model(cfg, 512, checkpoint_activations=True).train()
    opt = K.GRAD_SINK = FlatAdam(m, lr=1e-3, betas=(BETA1, BETA2), bucket_bytes=1 << 20)      # (bias corrections exact at every step)
    K.DROPOUT.step = 0
    assert len(opt.buckets) > 1
    return m, opt


def _train(m, opt, rank=0, steps=2):
    rng = np.random.default_rng(100 + rank)
    for _ in range(steps):
        enc = torch.from_numpy(rng.integers(5, 512, size=(8, 64))).cuda(); dec = torch.from_numpy(rng.integers(5, 512, size=(8, 32))).cuda()
        opt.zero_grad()
        logits, _ = m(enc, dec)
        logits.float().square().mean().backward()
        opt.finish()
        opt.step()


@pytest.fixture()
def sink():
    from emdr2_amd.model import kernels as K
    yield K
    K.GRAD_SINK = None
    K.DROPOUT.step = 0


def test_flat_adam_param_stats_after_a_real_step_against_torch_float64(sink):
    m, opt = _build()
    assert not hasattr(opt, "_pstats")                                   # never asked: no buffer
    _train(m, opt)
    state = [b[k].clone() for b in opt.buckets for k in ("master", "grad", "m", "v", "work")]
    stats = opt.param_stats()
    assert all(torch.equal(x, b[k]) for x, (b, k) in zip(state, [(b, k) for b in opt.buckets for k in ("master", "grad", "m", "v", "work")]))
    assert stats["step"] == opt.step_count == 2 and stats["grads_current"] is True and "learning rate" in stats["lr_note"]
    names = dict(m.named_parameters())
    assert set(stats["params"]) == set(names)
    bc1, bc2 = (float(x) for x in R.bias_corrections(BETA1, BETA2, opt.step_count))        # 0.75, 0.4375
    idle = []
    for name, r in stats["params"].items():
        p = names[name]
        g, w = opt.grad_view(p).double(), p.data.double()
        mm, vv = (t.double() for t in opt._moments(p))
        d = (mm / bc1) / ((vv / bc2).sqrt() + float(np.float32(opt.eps)))
        assert r["n"] == p.numel() and r["active"] == (opt.count[p] > 0)
        # a float64 sum in torch's order against the stated one: n * 2^-53 relative, far inside 1e-12; d in fp32 on the device: 2e-6
        for key, ref, tol in (("grad_sq", g.square().sum(), 1e-12), ("weight_sq", w.square().sum(), 1e-12), ("direction_sq", d.square().sum(), 2e-6)):
            assert abs(r[key] - float(ref)) <= tol * float(ref), (name, key, r[key], float(ref))
        assert r["grad_norm"] == r["grad_sq"] ** 0.5 and r["weight_norm"] == r["weight_sq"] ** 0.5
        assert r["direction_rms"] == (r["direction_sq"] / r["n"]) ** 0.5
        assert r["max_abs_grad"] == float(g.abs().max()) and r["max_abs_weight"] == float(w.abs().max())
        assert r["grad_zeros"] == int((g == 0).sum()) and r["grad_nonfinite"] == 0
        if not r["active"]:
            idle.append(name)
            assert r["grad_sq"] == 0.0 and r["direction_sq"] == 0.0 and r["max_abs_grad"] == 0.0 and r["grad_zeros"] == r["n"]
            assert r["weight_sq"] > 0.0                                  # (its weights are there all the same)
    assert idle and all("tokentype" in name for name in idle)            # the reader's unused token-type table
    # the global sum against the step's own fp32 norm: per-thread runs of the norm kernel at this size are under 16 terms
    total, gsq = sum(r["grad_sq"] for r in stats["params"].values()), float(opt._gsq)
    print("sum of grad_sq %.17g, the step's fp32 sum %.9g, relative %.3g" % (total, gsq, abs(total - gsq) / gsq))
    assert abs(total - gsq) <= 1e-5 * gsq
    assert opt.param_stats() == stats                                    # the same buckets: the same words
    opt.zero_grad()
    after = opt.param_stats()
    assert after["grads_current"] is False and after["step"] == 2
    assert all(r["grad_sq"] == 0.0 for r in after["params"].values())    # (zero_grad() has filled the buckets)
    assert all(after["params"][k]["weight_sq"] == r["weight_sq"] and after["params"][k]["direction_sq"] == r["direction_sq"]
               for k, r in stats["params"].items())


# ---- (f) two data-parallel ranks on the one GPU --------------------------------------------------------------------------------------------
def _rank(rank, world, port, out_dir):
    _init(rank, world, port, "gloo")
    from emdr2_amd.model import kernels as K
    m, opt = _build()
    _train(m, opt, rank=rank)                                            # different data per rank, the same averaged gradients
    words = opt.param_stats_words().cpu()
    stats = opt.param_stats()
    torch.save({"words": words, "stats": stats}, os.path.join(out_dir, "r%d.pt" % rank))
    K.GRAD_SINK = None
    torch.distributed.destroy_process_group()


def test_two_ranks_hold_the_same_table_bit_for_bit(tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_rank, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(str(tmp_path), "r%d.pt" % r), weights_only=False) for r in (0, 1))
    assert r0["words"].shape[1] == 8 and r0["words"].shape[0] == len(r0["stats"]["params"])
    assert torch.equal(r0["words"], r1["words"])
    assert r0["stats"] == r1["stats"] and r0["stats"]["grads_current"]
    assert sum(r["grad_sq"] for r in r0["stats"]["params"].values()) > 0.0
