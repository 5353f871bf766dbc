"""Round 6: annlite_rerank_topk -- the exact re-rank of candidate lists (GPU analogue of FlatIndex.search,
annlite/core/index/flat_index.py:15-39; hnswlib space_l2.h / space_ip.h) fused with the top-k -- against the steps it replaces:
annlite_exact_gather_dist -> masking -> annlite_topk_rows -> gather of the ids -> sqrt.  Bit for bit."""
import numpy as np
import pytest

from _refs import bitmap as _bitmap, fp32_chain_bound
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


@pytest.mark.parametrize('metric', [1, 2, 3])
@pytest.mark.parametrize('D,R,k', [(128, 128, 10), (64, 128, 10), (96, 50, 64), (768, 200, 16), (20, 7, 10), (128, 64, 1), (130, 129, 33)])
def test_fused_rerank_equals_gather_topk_gather(ops, metric, D, R, k):
    import torch

    rs = np.random.RandomState(D + R + k + metric)
    N, B = 5000, 37
    x = rs.randn(N, D).astype(np.float32)
    x[100:140] = x[100]  # ties: the position in the list decides
    q = rs.randn(B, D).astype(np.float32)
    cand = rs.randint(0, N, size=(B, R)).astype(np.int64)
    cand[:, : min(R, 30)] = rs.randint(100, 140, size=(B, min(R, 30)))
    cand[rs.rand(B, R) < 0.1] = -1
    cand[0, :] = -1            # a query without candidates
    cand[1, 1:] = -1           # ... with one
    cand[2, rs.randint(0, R)] = N + 3  # beyond the table
    valid = rs.rand(N) < 0.85
    bits = np.zeros(((N + 31) // 32 + 2) * 32, bool)
    bits[:N] = valid
    vb = ops.to_dev(np.packbits(bits.reshape(-1, 32), axis=1, bitorder='little').view(np.int32).reshape(-1))
    xd, qd, cd = ops.to_dev(x), ops.to_dev(q), ops.to_dev(cand)
    valid_d = ops.to_dev(valid)
    for vbits in (None, vb):
        for sqrt in (False, True):
            fd, fi = ops.rerank_topk(metric, qd, xd, cd, k, valid_bits=vbits, sqrt=sqrt)
            c2 = cd.clone()
            c2[c2 >= N] = -1
            if vbits is not None:
                ok = (c2 >= 0) & valid_d[c2.clamp(min=0)]
                c2 = torch.where(ok, c2, torch.full_like(c2, -1))
            exact = ops.exact_gather_dist(metric, qd, xd, c2)
            kk = min(k, R)
            d, pos = ops.topk_rows(exact, kk)
            i = torch.gather(c2, 1, pos.clamp(min=0))
            i = torch.where((pos < 0) | torch.isinf(d), torch.full_like(i, -1), i)
            if sqrt:
                d = torch.sqrt(d)
            if kk < k:
                d = torch.cat([d, torch.full((B, k - kk), float('inf'), device=d.device)], dim=1)
                i = torch.cat([i, torch.full((B, k - kk), -1, dtype=torch.int64, device=i.device)], dim=1)
            torch.cuda.synchronize()
            assert np.array_equal(fi.cpu().numpy(), i.cpu().numpy()), (metric, vbits is not None, sqrt)
            assert np.array_equal(fd.cpu().numpy().view(np.uint32), d.cpu().numpy().view(np.uint32))
    # and against numpy, loosely (the sums are fp32 in another order)
    fd, fi = ops.rerank_topk(metric, qd, xd, cd, k)
    fd, fi = fd.cpu().numpy(), fi.cpu().numpy()
    for b in (3, 17):
        ok = fi[b] >= 0
        ref = ((x[fi[b][ok]] - q[b]) ** 2).sum(1) if metric == 1 else 1.0 - x[fi[b][ok]] @ q[b]
        assert np.allclose(fd[b][ok], ref, rtol=1e-4, atol=1e-4)


def _pairs_rerank():
    Ds, Rs, ks = [1, 63, 64, 65, 768], [1, 63, 64, 65, 200], [1, 10, 64]
    return [(D, R, ks[(i + j) % len(ks)]) for i, D in enumerate(Ds) for j, R in enumerate(Rs)]


@pytest.mark.parametrize('metric', [1, 2, 3])
def test_fused_rerank_returns_the_float64_nearest(ops, metric):
    """Against float64: the returned ids are the k nearest valid candidates, ranks may differ from float64's only between
    candidates whose float64 distances lie within the fp32 summation bound of each other, and every distance lies within that
    bound of float64.  Bound per (query, candidate), terms t_j = (x_j - q_j)^2 (EUCLIDEAN) or x_j q_j: the kernel sums
    ceil(D / 64) terms per lane with fma, then a 6-level butterfly, so |error| <= (2 D + 4) u sum|t_j| + u |d| (u = 2^-24; the
    2 D covers the chains and the rounding of x_j - q_j, the last term 1 - s): ``_refs.fp32_chain_bound``."""
    for D, R, k in _pairs_rerank():
        rs = np.random.RandomState(1000 * metric + 10 * D + R)
        N, B = 3000, 6
        x = rs.randn(N, D).astype(np.float32)
        q = rs.randn(B, D).astype(np.float32)
        if metric == 3:
            x = (x / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
            q = (q / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
        cand = np.stack([rs.choice(N, R, replace=False) for _ in range(B)]).astype(np.int64)
        cand[rs.rand(B, R) < 0.15] = -1
        cand[0, :] = -1                      # no valid candidate
        if R > 1:
            cand[1, R - 1] = N + 5           # beyond the table: not a candidate
        fd, fi = ops.rerank_topk(metric, ops.to_dev(q), ops.to_dev(x), ops.to_dev(cand), k)
        fd, fi = fd.cpu().numpy(), fi.cpu().numpy()
        for b in range(B):
            ids = cand[b][(cand[b] >= 0) & (cand[b] < N)]
            x64, q64 = x[ids].astype(np.float64), q[b].astype(np.float64)
            terms = (x64 - q64) ** 2 if metric == 1 else x64 * q64
            d64 = terms.sum(1) if metric == 1 else 1.0 - terms.sum(1)
            tol = fp32_chain_bound(terms, d64, D)
            kk = min(k, ids.size)
            order = np.argsort(d64, kind='stable')
            pos = {int(r): j for j, r in enumerate(ids)}
            got = fi[b, :kk]
            assert (fi[b, kk:] == -1).all() and np.isinf(fd[b, kk:]).all(), (metric, D, R, k, b)
            assert len(set(got.tolist())) == kk and all(int(r) in pos for r in got), (metric, D, R, k, b)
            j_got = np.array([pos[int(r)] for r in got], dtype=np.int64)
            j_true = order[:kk]
            # the candidate returned at rank r is as near as float64's rank-r candidate, up to both bounds
            assert (np.abs(d64[j_got] - d64[j_true]) <= tol[j_got] + tol[j_true]).all(), (metric, D, R, k, b)
            assert (np.abs(fd[b, :kk].astype(np.float64) - d64[j_got]) <= tol[j_got]).all(), (metric, D, R, k, b)
            assert (np.diff(fd[b, :kk]) >= 0).all()


@pytest.mark.parametrize('metric', [1, 2, 3])
@pytest.mark.parametrize('D', [20, 130])
def test_fused_rerank_padding_zero_distances_duplicates_and_non_finite_vectors(ops, metric, D):
    """The inputs the random cases lack: lists of -1 (some, all), k above the number of valid candidates, a bitmap that deletes
    the nearest row, vectors EQUAL to the query (distance exactly 0 under every metric: the query is a unit basis vector),
    the same vector under several ids (the earlier list position wins: the documented order of the fused kernel, which for an
    ascending list is the lower id), one NaN and one inf coordinate.  WHICH rows may come back: float64 distances, within the
    fp32 summation bound of the test above.  Their VALUES and order: annlite_exact_gather_dist's bits (the five-launch
    path), selected here in numpy -- NaN last (behind the +inf of a -1 entry too), ties by position, a +inf distance is reported as
    (+inf, -1)."""
    rs = np.random.RandomState(10 * D + metric)
    N, B, R = 60, 7, 70
    x = rs.randn(N, D).astype(np.float32)
    q = rs.randn(B, D).astype(np.float32)
    if metric == 3:
        x = (x / np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
        q = (q / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    q[0] = 0
    q[0, 3] = 1.0
    q[1] = q[0]
    x[10] = x[11] = x[40] = q[0]          # distance 0 to query 0, three ids
    x[5] = x[6] = x[7] = x[30]            # one vector, four ids
    x[20, D - 1] = np.nan
    x[21, 0] = np.inf
    x[22, 3] = -np.inf
    cand = np.stack([rs.permutation(N) for _ in range(B)]).astype(np.int64)
    cand = np.concatenate([cand, cand[:, :R - N]], axis=1)   # R > N: every row at least once, ten of them twice
    cand[0] = np.concatenate([np.arange(N), np.arange(R - N)])  # ascending ids: position order is id order
    cand[1] = cand[0][::-1]                                     # descending: the HIGHER id stands first and wins
    cand[2, :] = -1                                             # nothing
    cand[3, 1:] = -1                                            # one candidate
    cand[3, 0] = 20                                             # ... the NaN vector
    cand[4, rs.rand(R) < 0.8] = -1
    cand[5, 5:] = -1
    valid = np.ones(N, bool)
    valid[[10, 30, 44]] = False                                 # the nearest row of query 0 and one of the duplicates
    xd, qd, cd = ops.to_dev(x), ops.to_dev(q), ops.to_dev(cand)
    for use_valid in (False, True):
        c2 = cand.copy()
        if use_valid:
            c2[(c2 >= 0) & ~valid[np.clip(c2, 0, N - 1)]] = -1
        exact = ops.exact_gather_dist(metric, qd, xd, ops.to_dev(c2)).cpu().numpy()
        for k in (1, 10, 64):
            fd, fi = ops.rerank_topk(metric, qd, xd, cd, k, valid_bits=ops.to_dev(_bitmap(valid)) if use_valid else None)
            fd, fi = fd.cpu().numpy(), fi.cpu().numpy()
            for b in range(B):
                nan = np.isnan(exact[b])
                o = np.lexsort((np.arange(R), np.where(nan, np.float32(0), exact[b]), nan))[:k]
                wd = exact[b][o]
                wi = np.where(wd == np.inf, -1, c2[b][o])
                assert np.array_equal(fi[b], wi), (metric, D, use_valid, k, b, fi[b][:8], wi[:8])
                assert np.array_equal(fd[b], wd, equal_nan=True), (metric, D, use_valid, k, b)
                fin = ~np.isnan(wd)
                assert np.array_equal(fd[b][fin].view(np.uint32), wd[fin].view(np.uint32))
                # float64: the rows returned are the nearest valid candidates
                pos = np.nonzero(c2[b] >= 0)[0]
                with np.errstate(all='ignore'):
                    x64, q64 = x[c2[b][pos]].astype(np.float64), q[b].astype(np.float64)
                    terms = (x64 - q64) ** 2 if metric == 1 else x64 * q64
                    d64 = terms.sum(1) if metric == 1 else 1.0 - terms.sum(1)
                    tol = fp32_chain_bound(terms, d64, D)
                # numbers below +inf first; then everything at +inf -- such candidates and every -1 / deleted position alike,
                # reported as (+inf, -1) --; NaN distances behind those (numpy's order)
                n_nan = int(np.isnan(d64).sum())
                n_num = int((d64 < np.inf).sum())
                n_inf = R - n_num - n_nan
                assert (fi[b] >= 0).sum() == min(k, n_num) + min(max(k - n_num - n_inf, 0), n_nan), (metric, D, use_valid, k, b)
                kk = min(k, n_num)
                if kk == 0:
                    continue
                n64 = np.isnan(d64)
                o64 = np.lexsort((np.where(n64, 0.0, d64), n64))
                last = o64[kk - 1]
                if not np.isfinite(d64[last]):
                    continue  # (the last number is -inf: only exact ties qualify, checked above)
                got = {int(r) for r in fi[b] if r >= 0}
                for j, p in enumerate(pos):
                    if int(c2[b][p]) in got and np.isfinite(d64[j]):
                        assert d64[j] <= d64[last] + tol[j] + tol[last], (metric, D, use_valid, k, b, int(c2[b][p]))
            if k == 64:  # the vectors equal to the query: distance exactly 0, in list order (query 1: the list reversed)
                want0 = ([11, 40], [40, 11]) if use_valid else ([10, 11, 40], [40, 11, 10])
                for b in (0, 1):
                    zero = [int(r) for r in fi[b][fd[b] == 0]]
                    assert [r for r in zero if r in (10, 11, 40)][:len(want0[b])] == want0[b], (metric, D, use_valid, b, zero)
