"""The float graph walk (annlite_graph_f32_search, graph_f32.hip) pinned BIT FOR BIT against a plain restatement of its order.

The order is that of the PQ walk one node at a time (tests/test_graph_pair.py ``walk_restated`` with width 1, restated here): seeds
scanned flat in rounds of 64, the best unexpanded entry expanded, a step's unseen neighbours (ids < N) tested against the list's
worst entry BEFORE any of them is inserted, the walk over when the first min(ef, 64 E) entries hold no unexpanded node.  What
differs is the distance: ``ops.exact_gather_dist`` over all rows is the oracle -- the kernel's distances carry its bits -- and the
list is ordered by (``f32_key(distance)``, node id): negative distances (INNER_PRODUCT) ascend, NaN sorts behind +inf."""
import numpy as np
import pytest

from _refs import bitmap, f32_key
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

EUCLIDEAN, INNER_PRODUCT, COSINE = 1, 2, 3
N, B, N_SEEDS = 3000, 10, 150


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _random_graph(rs, n, L, full_frac=0.6):
    links = np.zeros((n, L + 1), np.uint32)
    cnt = np.where(rs.rand(n) < full_frac, L, rs.randint(0, L + 1, n)).astype(np.uint32)  # ragged and empty lists
    links[:, 0] = cnt
    nb = rs.randint(0, n, size=(n, L)).astype(np.uint32)
    near = (np.arange(n)[:, None] + rs.randint(1, 50, size=(n, L))) % n
    nb = np.where(rs.rand(n, L) < 0.7, near, nb).astype(np.uint32)
    nb[rs.rand(n, L) < 0.002] = n + 5  # beyond the table: never followed
    nb[:, 1] = np.where(rs.rand(n) < 0.05, nb[:, 0], nb[:, 1])  # a neighbour listed twice
    links[:, 1:] = nb
    return links.view(np.int32)


def _key_to_bits(k):
    """inverse of the list's key: the float's own bits (the canonical NaN for the NaN key)"""
    k = int(k)
    return k ^ 0x80000000 if k & 0x80000000 else k ^ 0xffffffff


def walk_restated(links, seeds, keys, ef, valid=None):
    """One query.  ``links`` u32 [N, L+1] (count, ids), ``keys`` u64 [N]: f32_key of the query's distance to every row.
    Returns (ids i64 [ef], distance bits u32 [ef])."""
    n = keys.shape[0]
    E = 1 if ef <= 64 else 2 if ef <= 128 else 4  # registers per lane of the kernel's list
    slots, cap = 64 * E, min(ef, 64 * E)
    lst = []  # sorted [(key, node, expanded)]: the kernel's list of 64 E entries, `cap` of them live
    seen = set()

    def offer(nodes):
        if not len(nodes):
            return
        worst = (lst[cap - 1][0], lst[cap - 1][1]) if len(lst) >= cap else (1 << 40, 1 << 40)
        new = [(int(keys[v]), int(v), False) for v in nodes if (int(keys[v]), int(v)) < worst]
        lst.extend(new)
        lst.sort(key=lambda t: (t[0], t[1]))
        del lst[slots:]

    seeds = [int(s) for s in seeds]
    for s0 in range(0, len(seeds), 64):
        offer([s for s in seeds[s0:s0 + 64] if s < n])
    for t in lst:
        seen.add(t[1])
    while True:
        pick = [i for i, t in enumerate(lst[:cap]) if not t[2]][:1]
        if not pick:
            break
        i = pick[0]
        lst[i] = (lst[i][0], lst[i][1], True)
        fresh = []
        row = links[lst[i][1]]
        for nb in row[1:1 + int(row[0])]:
            nb = int(nb)
            if nb < n and nb not in seen:
                seen.add(nb)
                fresh.append(nb)
        offer(fresh)
    ids = np.full(ef, -1, np.int64)
    bits = np.full(ef, np.float32(np.inf).view(np.uint32), np.uint32)
    for i, t in enumerate(lst[:cap]):
        if valid is None or valid[t[1]]:
            ids[i] = t[1]
            bits[i] = _key_to_bits(t[0])
    return ids, bits


SHAPES = [(128, 32, 128), (64, 32, 64), (3, 5, 10), (200, 17, 33), (128, 32, 129), (128, 32, 200), (768, 24, 256), (128, 64, 100)]
CASES = [(EUCLIDEAN, *s) for s in SHAPES] + [(m, *s) for m in (INNER_PRODUCT, COSINE) for s in SHAPES[:2]]


@pytest.mark.parametrize('metric,D,L,ef', CASES)
def test_float_walk_equals_its_restatement(ops, metric, D, L, ef):
    import torch

    rs = np.random.RandomState(metric * 100003 + D * 1000 + L * 7 + ef)
    links = _random_graph(rs, N, L)
    x = rs.randn(N, D).astype(np.float32)
    x[1000:1040] = x[1000]  # exact ties inside the walk: the key's low word (the node id) decides
    q = rs.randn(B, D).astype(np.float32)
    q[2] = x[77]  # a stored row as its own query
    if metric == COSINE:  # (the index stores and asks normalised rows; the kernel computes 1 - <q, x> on what it is given)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[4, D // 2] = np.nan
    q[7, 0] = np.inf
    seeds = rs.choice(N, N_SEEDS, replace=False).astype(np.int32)  # three rounds of 64, the last one partial
    valid = rs.rand(N) < 0.9
    x_d, q_d, links_d, seeds_d = ops.to_dev(x), ops.to_dev(q), ops.to_dev(links), ops.to_dev(seeds)
    vb = ops.to_dev(bitmap(valid))
    all_rows = torch.arange(N, device='cuda', dtype=torch.int64)[None, :].expand(B, N).contiguous()
    dist = ops.exact_gather_dist(metric, q_d, x_d, all_rows).cpu().numpy()  # the oracle: the bits every kernel distance carries
    if metric == INNER_PRODUCT:
        assert (dist[0] < 0).sum() > N // 10  # negative distances: the key, not the float's bits, orders them
    if metric == EUCLIDEAN:
        assert dist[2, 77] == 0.0
    assert np.isnan(dist[4]).all() and not np.isfinite(dist[7]).any()
    keys = f32_key(dist)
    lk = links.view(np.uint32)
    for vbits, vmask in ((None, None), (vb, valid)):
        gi, gd = ops.graph_f32_search(metric, q_d, x_d, links_d, seeds_d, ef, valid_bits=vbits)
        torch.cuda.synchronize()
        gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
        for b in range(B):
            ri, rbits = walk_restated(lk, seeds, keys[b], ef, vmask)
            assert np.array_equal(gi[b], ri), (vmask is not None, b)
            assert np.array_equal(gd[b].view(np.uint32), rbits), (vmask is not None, b)


def test_float_walk_refuses_what_it_cannot_hold(ops):
    import torch

    rs = np.random.RandomState(1)
    links = ops.to_dev(_random_graph(rs, 100, 8))
    seeds = ops.to_dev(np.arange(10, dtype=np.int32))
    x = torch.zeros((100, 2049), dtype=torch.float32, device='cuda')
    with pytest.raises(Exception, match='2048'):
        ops.graph_f32_search(EUCLIDEAN, x[:2].contiguous(), x, links, seeds, 16)
    x = torch.zeros((100, 8), dtype=torch.float32, device='cuda')
    with pytest.raises(Exception, match='ef'):
        ops.graph_f32_search(EUCLIDEAN, x[:2].contiguous(), x, links, seeds, 257)
