"""The float graph walk over HALF-PRECISION rows (annlite_graph_f16_search, graph_f16.hip) pinned BIT FOR BIT: against the restated
walk order of tests/_refs.py over ``ops.exact_gather_dist_f16`` of all rows -- the bits every distance of the f16 graph carries --,
against ``ops.graph_f32_search`` over the widened rows, and against float64 within the fp32 summation bound.

The shapes are the ones at which the quarter-wave distance (16 lanes per row, four chains per lane, four rows per pass) can go
wrong: one active lane of a group (D = 4), a tail block that ends inside a group (D = 60), one that crosses 64 (D = 68, 200), partial
passes (L = 5, 17), more rows than one set of passes holds (L = 64), D = 2048, and the lane-strided path of every D % 4 != 0
(D = 1, 3, 130).  The data is tests/test_graph_f32_walk.py's, rounded to f16 on the host, with one row beyond the f16 range."""
import numpy as np
import pytest

from _refs import bitmap, f32_key, fp32_chain_bound, random_links, walk_restated
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


def _data(metric, D, L, n=N, n_seeds=N_SEEDS):
    rs = np.random.RandomState(metric * 100003 + D * 1000 + L * 7 + n + n_seeds)
    links = random_links(rs, n, L)
    x = rs.randn(n, D).astype(np.float32)
    x[1000:1040] = x[1000]  # exact ties inside the walk: the node id decides
    q = rs.randn(B, D).astype(np.float32)
    if metric == COSINE:
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    x[5, 0] = 70000.0  # beyond the f16 range: stored as +inf
    with np.errstate(over='ignore'):
        x16 = x.astype(np.float16)
    assert np.isposinf(x16[5, 0])
    q[2] = x16[77].astype(np.float32)  # a stored row as its own query
    q[4, D // 2] = np.nan
    q[7, 0] = np.inf
    seeds = rs.choice(n, n_seeds, replace=False).astype(np.int32)
    if 77 not in seeds:
        seeds[0] = 77  # (random links are no proximity graph: the row that is its own query is a seed)
    return links, x16, q, seeds, rs.rand(n) < 0.9


def _check(ops, metric, D, L, ef, chain_bound=False, **kw):
    import torch

    links, x16, q, seeds, valid = _data(metric, D, L, **kw)
    n = x16.shape[0]
    x_d, q_d, links_d, seeds_d = ops.to_dev(x16), ops.to_dev(q), ops.to_dev(links), ops.to_dev(seeds)
    assert x_d.dtype == torch.float16
    all_rows = torch.arange(n, device='cuda', dtype=torch.int64)[None, :].expand(B, n).contiguous()
    dist = ops.exact_gather_dist_f16(metric, q_d, x_d, all_rows).cpu().numpy()
    keys = f32_key(dist)
    lk = links.view(np.uint32)
    for vbits, vmask in ((None, None), (ops.to_dev(bitmap(valid)), valid)):
        gi, gd = ops.graph_f16_search(metric, q_d, x_d, links_d, seeds_d, ef, valid_bits=vbits)
        fi, fd = ops.graph_f32_search(metric, q_d, x_d.float(), links_d, seeds_d, ef, valid_bits=vbits)
        torch.cuda.synchronize()
        gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
        for b in range(B):
            ri, rbits = walk_restated(lk, seeds, keys[b], ef, vmask)
            assert np.array_equal(gi[b], ri), (vmask is not None, b)
            assert np.array_equal(gd[b].view(np.uint32), rbits), (vmask is not None, b)
        assert np.array_equal(gi, fi.cpu().numpy()) and np.array_equal(gd.view(np.uint32), fd.cpu().numpy().view(np.uint32))
    # (without the bitmap once more: under it row 77 may be blanked)
    gi, gd = ops.graph_f16_search(metric, q_d, x_d, links_d, seeds_d, ef)
    gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
    if metric == EUCLIDEAN:
        assert gi[2, 0] == 77 and gd[2, 0].view(np.uint32) == 0  # +0.0
    if chain_bound:
        x64 = x16.astype(np.float64)
        for b in range(B):
            ok = (gi[b] >= 0) & np.isfinite(gd[b])
            terms = (x64[gi[b][ok]] - q[b].astype(np.float64)) ** 2 if metric == EUCLIDEAN else x64[gi[b][ok]] * q[b].astype(np.float64)
            d64 = terms.sum(1) if metric == EUCLIDEAN else 1.0 - terms.sum(1)
            err = np.abs(gd[b][ok].astype(np.float64) - d64)
            assert (err <= fp32_chain_bound(terms, d64, D)).all(), b


SHAPES = [(128, 32, 128), (64, 32, 64), (4, 5, 10), (60, 17, 33), (68, 17, 33), (200, 32, 129), (768, 24, 256), (2048, 8, 32),
          (128, 64, 100), (1, 4, 8), (3, 5, 10), (130, 32, 64)]
CASES = [(EUCLIDEAN, *s) for s in SHAPES] + [(m, *s) for m in (INNER_PRODUCT, COSINE) for s in SHAPES[:2]]


@pytest.mark.parametrize('metric,D,L,ef', CASES)
def test_f16_walk_equals_restatement_gather_and_f32_twin(ops, metric, D, L, ef):
    _check(ops, metric, D, L, ef, chain_bound=D in (4, 768, 2048))


@pytest.mark.parametrize('n_seeds', [1, 64, 65])
def test_f16_walk_seed_sets(ops, n_seeds):
    _check(ops, EUCLIDEAN, 128, 32, 64, n_seeds=n_seeds)


def test_f16_walk_over_one_row(ops):
    import torch

    x = ops.to_dev(np.array([[1.0, 2.0, 3.0, 4.0]], np.float16))
    q = ops.to_dev(np.array([[1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 1.0, 4.0]], np.float32))
    links, seeds = ops.to_dev(np.zeros((1, 9), np.int32)), ops.to_dev(np.zeros(1, np.int32))
    gi, gd = ops.graph_f16_search(EUCLIDEAN, q, x, links, seeds, 10)
    torch.cuda.synchronize()
    assert np.array_equal(gi.cpu().numpy(), np.array([[0] + [-1] * 9] * 2))
    assert np.array_equal(gd.cpu().numpy(), np.array([[0.0] + [np.inf] * 9, [9.0] + [np.inf] * 9], np.float32))
