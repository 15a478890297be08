"""GPU: the all-exact fallback and the shard merge driven DIRECTLY, in both score formats (fp16: RNE_fp16(exact dot); fp32: RNE_fp32), against
the CPU oracle bit for bit.  Through `search` the all-exact path only runs for queries the fast path happens to flag; here every query is
selected, at the shapes where its kernels (csrc/mips_aux.hip: exact_scores_kernel<Fmt>, exact_select_kernel<Fmt>, merge_kernel<Fmt, Source>)
take another path: the smallest launch, fewer rows than k (padding), two passes through the 8-query key workspace, ties that straddle the
8,192-row collection round, and boundary-bucket ties at every radix level."""
import functools

import numpy as np
import pytest
import torch

import mips_cases
from oracle import mips_oracle as mo

pytestmark = pytest.mark.gpu


def _random_case(n, dim, nq, k):
    rng = np.random.default_rng(1000 * n + dim + nq)
    return dict(rows=rng.standard_normal((n, dim)).astype(np.float16), queries=rng.standard_normal((nq, dim)).astype(np.float16), k=k)


def _round_boundary_case():
    """Ten rows tie for the best score (2.0) at rows 8190..8199: the first two sit in the first 8,192-row collection round, the others
    in the second, and only the first five belong to the top-5 -- the count of equal keys already taken has to carry across the rounds."""
    n, dim = 8200, 64
    rows = 0.01 * np.random.default_rng(8200).standard_normal((n, dim))
    rows[:, 0] = 0.5
    rows[8190:] = 0.0
    rows[8190:, 0] = 2.0
    q = np.zeros((2, dim))
    q[:, 0] = 1.0
    return dict(rows=rows.astype(np.float16), queries=q.astype(np.float16), k=5)


CASES = {
    "n1": functools.partial(_random_case, 1, 64, 1, 1),                 # smallest launch
    "n37_k50": functools.partial(_random_case, 37, 64, 3, 50),          # fewer rows than k: slots 37..49 are padding
    "n300_k120": functools.partial(_random_case, 300, 96, 9, 120),      # 9 queries = passes of 8 + 1; MAX_TOPK-sized k; 12 segments < 64 lanes
    "n8200_round_boundary": _round_boundary_case,
    "exact_ties": mips_cases.case_exact_ties,                           # heavy ties in the boundary bucket of every radix level
}


@functools.lru_cache(maxsize=None)
def _case(name):
    c = CASES[name]()
    n = c["rows"].shape[0]
    ids = (np.random.default_rng(n).permutation(n) + 1).astype(np.int32)
    return c["rows"], c["queries"], c["k"], ids


def _oracle(rows, q, k, ids, f32):
    """(score bits, doc ids, rows) of the canonical top-k; the tail past the last row is (-inf, -1, -1)."""
    if f32:
        od, oi = mo.topk_f32(rows, q, k, ids=ids.astype(np.int64))
        _, orow = mo.topk_f32(rows, q, k)                               # (without an id map the oracle's ids are the rows)
        return od.view(np.uint32), oi, orow
    od, oi, orow = mo.topk(rows, q, k, ids=ids, return_rows=True)
    return od.view(np.uint16), oi.astype(np.int64), orow


def _shard(rows, ids, row_base=0):
    from emdr2_amd.data.emdr2_index import HipIndexShard
    sh = HipIndexShard(rows.shape[1], rows.shape[0], row_base)
    sh.append_rows(rows)
    sh.set_ids(ids)
    return sh


def _bits(t, f32):
    return t.cpu().numpy().view(np.uint32 if f32 else np.uint16)


@pytest.mark.parametrize("f32", [False, True], ids=["fp16", "fp32"])
@pytest.mark.parametrize("name", list(CASES))
def test_all_exact_path_matches_the_oracle_for_every_query(name, f32):
    rows, q, k, ids = _case(name)
    nq = q.shape[0]
    sh = _shard(rows, ids)
    dist = torch.zeros((nq, k), dtype=torch.float32 if f32 else torch.float16, device="cuda")
    idx = torch.full((nq, k), -7, dtype=torch.int32, device="cuda")
    row = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
    flags = torch.ones(nq, dtype=torch.int32, device="cuda")
    sh.search_exact(torch.from_numpy(q).cuda(), torch.arange(nq, dtype=torch.int32, device="cuda"), k, dist, idx, row, flags, f32)
    torch.cuda.synchronize()
    ob, oi, orow = _oracle(rows, q, k, ids, f32)
    assert np.array_equal(_bits(dist, f32), ob)
    assert np.array_equal(idx.cpu().numpy().astype(np.int64), oi)
    assert np.array_equal(row.cpu().numpy(), orow)
    assert (flags.cpu().numpy() == 0).all()
    if name == "n8200_round_boundary":
        assert np.array_equal(orow, np.tile(np.arange(8190, 8195), (nq, 1)))
    if name == "n37_k50":
        pad = 0xff800000 if f32 else 0xfc00
        assert (ob[:, 37:] == pad).all() and (oi[:, 37:] == -1).all() and (orow[:, 37:] == -1).all()


@pytest.mark.parametrize("f32", [False, True], ids=["fp16", "fp32"])
def test_array_merge_and_record_merge_equal_the_single_shard_search(f32):
    """Three 100-row shards (fewer rows than k = 120: every list ends in invalid slots) and one of 7 rows."""
    from emdr2_amd.data.emdr2_index import merge_shard_records, merge_shard_results
    rows300, q, k, _ = _case("n300_k120")
    rows = np.concatenate([rows300, np.random.default_rng(7).standard_normal((7, rows300.shape[1])).astype(np.float16)])
    ids = (np.random.default_rng(307).permutation(rows.shape[0]) + 1).astype(np.int32)
    qd = torch.from_numpy(q).cuda()
    search = lambda sh: (sh.search_f32 if f32 else sh.search)(qd, k)[:3]
    d1, i1, r1 = search(_shard(rows, ids))
    bounds = [(0, 100), (100, 200), (200, 300), (300, 307)]
    shards = [_shard(rows[lo:hi], ids[lo:hi], row_base=lo) for lo, hi in bounds]
    parts = [search(sh) for sh in shards]
    gathered = torch.stack([sh.search_records(qd, k, f32=f32)[0] for sh in shards])
    merged_arrays = merge_shard_results(*[torch.stack([p[j] for p in parts]) for j in range(3)])
    merged_records = merge_shard_records(gathered, f32=f32)
    torch.cuda.synchronize()
    for md, mi, mr in (merged_arrays, merged_records):
        assert md.dtype == d1.dtype
        assert np.array_equal(_bits(md, f32), _bits(d1, f32))
        assert torch.equal(mi, i1) and torch.equal(mr, r1)
