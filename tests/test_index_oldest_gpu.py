"""GPU: emdr2_mips_oldest_rows and HipIndexShard.oldest_rows against the numpy statement of the contract
(tests/test_index_oldest_cpu.oldest_rows_reference), bit for bit: the rows and all four report words.  Sizes: 1,000 (one slab, a partial
chunk) and 9,001 (nine slabs) are the sizes of the generation tests; 70,001 rows make 69 slabs of 1,024 rows, so the sums over the
slabs in front and a cut inside a late slab are exercised.  Stamp patterns: one value (the order is the row order); two values with the
cut inside the run of ties, in the first slab and in the last; small clustered values (one bin in the upper two digits); full 31-bit
values with 0 and 2^31 - 1 (every digit decides); strictly descending (the oldest rows are the last ones)."""
import numpy as np
import pytest
import torch

from tests.test_index_generations_gpu import _dev_rows, _stamped
from tests.test_index_oldest_cpu import oldest_rows_reference

pytestmark = pytest.mark.gpu
SIZES = (1000, 9001, 70001)
PATTERNS = ("equal", "two_first", "two_last", "small", "full", "descending")
MASK = (1 << 64) - 1


def _stamps(pattern, n, seed):
    rng = np.random.default_rng(seed)
    if pattern == "equal":
        return np.full(n, 7, dtype=np.int64)
    if pattern == "two_first":                                           # ten old rows, then the cut falls among the fives of the first slab
        s = np.full(n, 5, dtype=np.int64)
        s[rng.choice(n, size=10, replace=False)] = 3
        return s
    if pattern == "two_last":                                            # the old rows are the last 200: the cut falls among them, in the last slab
        s = np.full(n, 5, dtype=np.int64)
        s[n - 200:] = 3
        return s
    if pattern == "small":
        return rng.integers(0, 51, size=n)
    if pattern == "full":
        s = rng.integers(0, 1 << 31, size=n)
        s[rng.choice(n, size=4, replace=False)] = [0, 0, (1 << 31) - 1, (1 << 31) - 1]
        return s
    assert pattern == "descending"
    return np.arange(n, 0, -1, dtype=np.int64) * 3


class _Device(object):
    def __init__(self):
        from emdr2_amd import _native
        import ctypes
        self.native, self.lib = _native, _native.lib()
        nbytes = ctypes.c_size_t()
        _native.check(self.lib.emdr2_mips_oldest_rows_workspace_bytes(max(SIZES), ctypes.byref(nbytes)), "workspace_bytes")
        self.ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")

    def __call__(self, gen, row_base, below, n_want, ws=None, raw=False):
        """gen: CUDA int32 stamps -> (rows int64 [n_want], the four report words as unsigned ints), or their bytes"""
        ws = self.ws if ws is None else ws
        rows = torch.full((n_want + 1,), -7, dtype=torch.int64, device="cuda")        # one slot more: nothing is written behind n_want
        info = torch.full((4,), -7, dtype=torch.int64, device="cuda")
        self.native.check(self.lib.emdr2_mips_oldest_rows(gen.data_ptr(), gen.numel(), row_base, below, n_want, rows.data_ptr() if n_want else None,
                                                          info.data_ptr(), ws.data_ptr(), ws.numel(), self.native.stream_ptr()), "oldest_rows")
        rows, info = rows.cpu().numpy(), info.cpu().numpy()
        assert rows[n_want] == -7
        if raw:
            return rows.tobytes() + info.tobytes()
        return rows[:n_want], [int(w) & MASK for w in info]


@pytest.fixture(scope="module")
def device():
    return _Device()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_device_selection_is_the_reference_bit_for_bit(device, n, pattern):
    stamps = _stamps(pattern, n, seed=n + len(pattern))
    gen = torch.from_numpy(stamps.astype(np.int32)).cuda()
    row_base = 0 if n == 1000 else (1 << 33) + 12345                     # global rows beyond 32 bits
    for below in (0, int(stamps.min()), int(np.median(stamps)), 1 << 31):
        for n_want in (0, 1, 64, n - 1, n):
            rows, info = device(gen, row_base, below, n_want)
            ref_rows, ref_info = oldest_rows_reference(stamps, n_want, below, row_base)
            what = (n, pattern, below, n_want)
            print("n %6d %-10s below %10d want %6d -> selected %6d eligible %6d max stamp %d" % (what + tuple(info[:3])))
            assert info == ref_info, what
            assert np.array_equal(rows, ref_rows), what


def test_no_rows_and_the_report_alone(device):
    gen = torch.zeros(4, dtype=torch.int32, device="cuda")
    rows, info = device(gen[:0], 5, 9, 0)
    assert rows.size == 0 and info == [0, 0, MASK, 0]
    rows, info = device(gen, 5, 9, 0)                                    # n_want == 0: how many rows are older than 9, nothing else
    assert info == [0, 4, MASK, 0]


@pytest.mark.parametrize("pattern", ("two_last", "full"))
def test_result_is_a_function_of_the_stamps_alone(device, pattern):
    n = 70001
    stamps = _stamps(pattern, n, seed=3)
    gen = torch.from_numpy(stamps.astype(np.int32)).cuda()
    below = int(np.quantile(stamps, 0.8)) + 1
    first = device(gen, 77, below, 5000, raw=True)
    assert device(gen, 77, below, 5000, raw=True) == first               # the workspace as the first call left it
    dirty = torch.full_like(device.ws, 0xFF)
    assert device(gen, 77, below, 5000, ws=dirty, raw=True) == first     # a workspace of garbage: the call clears what it needs
    ref_rows, ref_info = oldest_rows_reference(stamps, 5000, below, 77)
    assert first == np.append(ref_rows, -7).tobytes() + np.array(ref_info, dtype=np.uint64).tobytes()


def test_shard_oldest_rows_feeds_the_scattered_writer():
    from emdr2_amd.data.emdr2_index import HipIndexShard
    n, dim, base = 1000, 64, 5000
    rng = np.random.default_rng(11)
    m = rng.standard_normal((n, dim)).astype(np.float16)
    sh = _stamped(m, row_base=base)
    stamps = rng.integers(0, 6, size=n)
    sh.generation[:n] = torch.from_numpy(stamps.astype(np.int32)).cuda()
    g = 4
    rows, info = sh.oldest_rows(64, below=g)
    assert rows.dtype == torch.int64 and rows.is_cuda and tuple(rows.shape) == (64,) and info.dtype == torch.int64 and tuple(info.shape) == (4,)
    ref_rows, ref_info = oldest_rows_reference(stamps, 64, g, base)
    assert np.array_equal(rows.cpu().numpy(), ref_rows) and [int(w) & MASK for w in info.tolist()] == ref_info
    # the selected rows, written with the weights of generation g: exactly their stamps rise, and the shard is still a fresh build
    new = rng.standard_normal((64, dim)).astype(np.float16)
    sh.update_rows_at(rows - base, _dev_rows(new), generation=g, newest_wins=True)
    assert sh.kept_newer() == 0                                          # nothing selected is newer than g
    expect = stamps.copy()
    expect[ref_rows - base] = g
    assert np.array_equal(sh.generation.cpu().numpy()[:n].astype(np.int64), expect)
    m[ref_rows - base] = new
    assert np.array_equal(sh.rows(np.arange(n)).cpu().numpy(), m)
    audit = sh.audit()
    assert audit["sound"] and audit["canonical"], audit
    # fewer eligible rows than asked for: -1 behind them, which the writer skips; n is clamped to the shard
    rows, info = sh.oldest_rows(5000, below=1)
    zeros = np.nonzero(expect == 0)[0]
    assert tuple(rows.shape) == (n,) and info.tolist()[:2] == [zeros.size, zeros.size]
    assert np.array_equal(rows.cpu().numpy()[:zeros.size], base + zeros) and (rows[zeros.size:] == -1).all()
    rows, info = sh.oldest_rows(0, below=1 << 31)
    assert rows.numel() == 0 and info.tolist() == [0, n, -1, 0]
    for bad in (-1, (1 << 31) + 1):
        with pytest.raises(ValueError):
            sh.oldest_rows(8, below=bad)
    with pytest.raises(ValueError):
        sh.oldest_rows(-1, below=3)
    plain = HipIndexShard(dim, n, 0)
    plain.append_rows(m)
    with pytest.raises(ValueError):
        plain.oldest_rows(8, below=3)                                    # no stamps
    filling = HipIndexShard(dim, n, 0, generations=True)
    filling.append_rows(m[:500])
    with pytest.raises(ValueError):
        filling.oldest_rows(8, below=3)                                  # still being filled
