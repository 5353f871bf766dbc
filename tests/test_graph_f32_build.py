"""The float graph's build kernels (annlite_graph_f32_build_select / annlite_graph_f32_build_reverse, graph_f32.hip) against plain
restatements of their rules -- those of tests/test_graph_gpu_build.py (hnsw_host.cpp select_neighbors / connect), restated here with
the float distance: every distance is read from an N x N matrix of ``ops.exact_gather_dist`` bits, the numbers the kernels compare."""
import numpy as np
import pytest

from _refs import f32_key
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]
SENT = np.iinfo(np.int64).max
EUCLIDEAN, INNER_PRODUCT, COSINE = 1, 2, 3
N = 3000


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


_cache = {}


def _table(ops, D, metric):
    """N clustered rows with near-duplicates and exact duplicates, and their N x N distance matrix (computed once per shape)."""
    import torch

    if (D, metric) not in _cache:
        rs = np.random.RandomState(D * 10 + metric)
        centers = (2.0 * rs.randn(12, D)).astype(np.float32)
        x = (centers[rs.randint(0, 12, N)] + 0.3 * rs.randn(N, D)).astype(np.float32)
        near = rs.choice(N, 300, replace=False)
        x[near] = (x[rs.randint(0, N, 300)] * np.float32(1 + 2 ** -20)).astype(np.float32)  # near-duplicates
        dup = rs.choice(N, 300, replace=False)
        x[dup] = x[rs.randint(0, N, 300)]  # exact duplicates: distance 0 between candidates, ties
        if metric == COSINE:
            x /= np.linalg.norm(x, axis=1, keepdims=True)
        x_d = ops.to_dev(x)
        rows = torch.arange(N, device='cuda', dtype=torch.int64)[None, :].expand(N, N).contiguous()
        dm = ops.exact_gather_dist(metric, x_d, x_d, rows).cpu().numpy()
        assert np.array_equal(dm.view(np.uint32), dm.T.copy().view(np.uint32))  # the arithmetic is symmetric, bit for bit
        _cache[(D, metric)] = (x, x_d, dm)
    return _cache[(D, metric)]


def _select(dm, base, pool, m_max):
    """hnsw_host.cpp select_neighbors over a pool that is already in visiting order."""
    pool = [int(p) for p in pool if p >= 0 and p != base]
    if len(pool) <= m_max:
        return pool
    keep = []
    for c in pool:
        if len(keep) >= m_max:
            break
        tb = dm[base, c]
        if all(not (dm[k, c] < tb) for k in keep):
            keep.append(c)
    return keep


@pytest.mark.parametrize('metric,D,ef,keep', [(EUCLIDEAN, 32, 200, 16), (EUCLIDEAN, 100, 256, 12), (EUCLIDEAN, 32, 10, 16),
                                             (EUCLIDEAN, 100, 40, 4), (INNER_PRODUCT, 32, 200, 12), (COSINE, 100, 256, 16)])
def test_float_select_kernel_is_algorithm_4(ops, metric, D, ef, keep):
    import torch

    rs = np.random.RandomState(D + ef + metric)
    x, x_d, dm = _table(ops, D, metric)
    b = 37
    base0 = N - b
    cand = np.full((b, ef), -1, np.int64)
    for i in range(b):
        n_c = ef if i % 5 else rs.randint(0, ef + 1)  # ragged lists, some shorter than `keep`
        ids = rs.choice(base0, n_c, replace=False)
        # visiting order = the base point's distance, with a few holes and the point itself
        ids = ids[np.argsort(f32_key(dm[base0 + i, ids]), kind='stable')]
        cand[i, :n_c] = ids
        if n_c > 8:
            cand[i, rs.randint(0, n_c, 2)] = -1
            cand[i, rs.randint(0, n_c)] = base0 + i
    lpn = 32
    links = torch.zeros((N, lpn + 1), dtype=torch.int32, device='cuda')
    pairs = ops.graph_f32_build_select(metric, ops.to_dev(cand), base0, x_d, keep, links)
    torch.cuda.synchronize()
    lk, pr = links.cpu().numpy().view(np.uint32), pairs.cpu().numpy()
    pruned = 0
    for i in range(b):
        want = _select(dm, base0 + i, cand[i], keep)
        row = lk[base0 + i]
        assert int(row[0]) == len(want), (i, row[:8], want)
        assert row[1:1 + len(want)].tolist() == want, i
        got_pairs = [int(p) for p in pr[i] if p != SENT]
        assert got_pairs == [(t << 32) | (base0 + i) for t in want]
        real = [int(p) for p in cand[i] if p >= 0 and p != base0 + i]
        pruned += len(real) > keep and want != real[:keep]
    assert pruned > 0 or ef <= keep  # (the heuristic did reject candidates: the check is not the first-`keep` rule)
    assert not lk[:base0].any()  # nobody else's row is touched


@pytest.mark.parametrize('metric,D', [(EUCLIDEAN, 32), (EUCLIDEAN, 100), (INNER_PRODUCT, 32)])
def test_float_reverse_kernel_appends_dedupes_and_shrinks(ops, metric, D):
    import torch

    rs = np.random.RandomState(9 + D + metric)
    x, x_d, dm = _table(ops, D, metric)
    lpn, half = 32, 1000
    links = np.zeros((N, lpn + 1), np.uint32)
    links[:, 1:] = 7  # (slots beyond a count hold anything)
    targets = rs.choice(half, 120, replace=False)
    pairs = []
    want = {}
    shrunk = 0
    for t_i, t in enumerate(targets):
        c = [0, 5, 20, 31, 32, 32, 32][t_i % 7]
        cur = [int(v) for v in rs.choice(np.setdiff1d(np.arange(half), [t]), c, replace=False)]
        links[t, 0] = c
        links[t, 1:1 + c] = cur
        k = [1, 3, 12, 1, 1, 7, 40][(t_i // 7) % 7]
        src = [int(v) for v in rs.choice(np.arange(half, N), k, replace=False)]
        if cur and t_i % 3 == 0:
            src.append(cur[0])  # a source that is in the list already: dropped
        if t_i % 11 == 0:
            src.append(int(t))  # the target itself: dropped
        src = sorted(set(src))
        pairs += [(int(t) << 32) | s for s in src]
        pool = cur + [s for s in src[: 64 - c] if s not in cur and s != t]  # at most 64 - count sources are taken
        if len(pool) == len(cur):
            want[int(t)] = cur
        elif len(pool) <= lpn:
            want[int(t)] = pool
        else:
            kt = f32_key(dm[t])
            order = sorted(pool, key=lambda v: (int(kt[v]), v))
            want[int(t)] = _select(dm, int(t), order, lpn)
            shrunk += 1
    assert shrunk >= 20
    keys = np.array(sorted(pairs), dtype=np.int64)
    tg = keys >> 32
    bounds = np.concatenate([[0], np.nonzero(np.diff(tg))[0] + 1, [len(keys)]]).astype(np.int64)
    links_d = ops.to_dev(links.view(np.int32))
    ops.graph_f32_build_reverse(metric, ops.to_dev(keys), ops.to_dev(bounds), x_d, links_d)
    torch.cuda.synchronize()
    got = links_d.cpu().numpy().view(np.uint32)
    for t, w in want.items():
        assert int(got[t, 0]) == len(w), (t, got[t, :6], w[:6])
        assert got[t, 1:1 + len(w)].tolist() == w, t
    untouched = np.setdiff1d(np.arange(N), targets)
    assert np.array_equal(got[untouched], links[untouched])  # rows nobody links are untouched
