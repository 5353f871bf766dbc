"""The build kernels and the admit walk of the float graph over HALF-PRECISION rows (graph_f16.hip) against their f32 twins over the
widened rows.  The f32 kernels are pinned to restatements by tests/test_graph_f32_build.py and tests/test_graph_f32_admit_walk.py, and
widening an f16 value is exact: equality with the twin, bit for bit, is the sharp check.  D = 4 (one active lane of a quarter-wave
group), 68 (a tail block that ends inside a group), 130 (the lane-strided path), 768; here the "query" is itself an f16 row."""
import numpy as np
import pytest

from _refs import bitmap, random_links
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

EUCLIDEAN, INNER_PRODUCT, COSINE = 1, 2, 3
N = 2000
CASES = [(m, D) for m in (EUCLIDEAN, INNER_PRODUCT, COSINE) for D in (4, 68, 130, 768)]


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _rows(ops, metric, D):
    """(rs, x16 on the host, the f16 table, the widened f32 table)"""
    rs = np.random.RandomState(metric * 1009 + D)
    x = rs.randn(N, D).astype(np.float32)
    x[300:320] = x[300]  # exact ties
    if metric == COSINE:
        x /= np.linalg.norm(x, axis=1, keepdims=True)
    x16 = x.astype(np.float16)
    x_d = ops.to_dev(x16)
    return rs, x16, x_d, x_d.float()


def _near(x16, metric, base):
    x = x16.astype(np.float32)
    return -(x @ x[base]) if metric == INNER_PRODUCT else ((x - x[base]) ** 2).sum(1)


@pytest.mark.parametrize('keep,lpn', [(2, 4), (64, 64)])
@pytest.mark.parametrize('metric,D', CASES)
def test_f16_select_equals_f32_select_over_widened_rows(ops, metric, D, keep, lpn):
    import torch

    rs, x16, x_d, xf_d = _rows(ops, metric, D)
    b, ef = 37, 256
    base0 = N - b
    cand = np.full((b, ef), -1, np.int64)
    for i in range(b):
        n_c = ef if i % 5 else rs.randint(0, ef + 1)  # a 256-entry pool, some ragged, some shorter than `keep`
        ids = rs.choice(base0, n_c, replace=False)
        cand[i, :n_c] = ids[np.argsort(_near(x16, metric, base0 + i)[ids], kind='stable')]
        if n_c > 8:
            cand[i, rs.randint(0, n_c, 3)] = base0 + i                  # the base point, more than once
            cand[i, rs.randint(0, n_c, 2)] = (N + 5, 0xfffffffe)        # ids beyond the table
            cand[i, rs.randint(0, n_c)] = -1
    cand_d = ops.to_dev(cand)
    got_links = torch.zeros((N, lpn + 1), dtype=torch.int32, device='cuda')
    want_links = torch.zeros_like(got_links)
    got = ops.graph_f16_build_select(metric, cand_d, base0, x_d, keep, got_links)
    want = ops.graph_f32_build_select(metric, cand_d, base0, xf_d, keep, want_links)
    torch.cuda.synchronize()
    assert torch.equal(got_links, want_links) and torch.equal(got, want)
    assert int(want_links[base0:, 0].max()) >= 2  # (lists were written)


@pytest.mark.parametrize('lpn', [1, 32])
@pytest.mark.parametrize('metric,D', CASES)
def test_f16_reverse_equals_f32_reverse_over_widened_rows(ops, metric, D, lpn):
    import torch

    rs, x16, x_d, xf_d = _rows(ops, metric, D)
    half = N // 2
    links = np.zeros((N, lpn + 1), np.uint32)
    links[:, 1:] = 7  # (slots beyond a count hold anything)
    pairs = []
    for t_i, t in enumerate(rs.choice(half, 120, replace=False)):
        c = [0, lpn // 2, lpn, lpn, lpn + 5][t_i % 5]  # (a count above lpn is read as lpn)
        links[t, 1:1 + min(c, lpn)] = rs.choice(np.setdiff1d(np.arange(half), [t]), min(c, lpn), replace=False)
        links[t, 0] = c
        src = rs.choice(np.arange(half, N), [1, 3, 12, 40][(t_i // 5) % 4], replace=False)
        pairs += [(int(t) << 32) | int(s) for s in src]
    keys = np.array(sorted(pairs), dtype=np.int64)
    bounds = np.concatenate([[0], np.nonzero(np.diff(keys >> 32))[0] + 1, [len(keys)]]).astype(np.int64)
    bounds = np.sort(np.concatenate([bounds, bounds[::7]]))  # every seventh bound twice: empty segments
    keys_d, seg_d = ops.to_dev(keys), ops.to_dev(bounds)
    got, want = ops.to_dev(links.view(np.int32)), ops.to_dev(links.view(np.int32))
    ops.graph_f16_build_reverse(metric, keys_d, seg_d, x_d, got)
    ops.graph_f32_build_reverse(metric, keys_d, seg_d, xf_d, want)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert not torch.equal(want, ops.to_dev(links.view(np.int32)))  # (lists were rewritten)


@pytest.mark.parametrize('metric,D', CASES)
def test_f16_admit_walk_equals_f32_admit_walk_over_widened_rows(ops, metric, D):
    import torch

    rs, x16, x_d, xf_d = _rows(ops, metric, D)
    links_d = ops.to_dev(random_links(rs, N, 32))
    seeds_d = ops.to_dev(rs.choice(N, 150, replace=False).astype(np.int32))
    q_d = ops.to_dev(np.concatenate([rs.randn(9, D).astype(np.float32), x16[77:78].astype(np.float32)]))
    admit = ops.to_dev(bitmap(rs.rand(N) < 0.3))
    out = []
    for fn, rows in ((ops.graph_f16_search_admit, x_d), (ops.graph_f32_search_admit, xf_d)):
        worst = torch.empty(10, dtype=torch.float32, device='cuda')
        ids, dist = fn(metric, q_d, rows, links_d, seeds_d, 128, 64, admit, route_worst=worst)
        out.append((ids, dist.view(torch.int32), worst.view(torch.int32)))
    torch.cuda.synchronize()
    for g, w in zip(*out):
        assert torch.equal(g, w)
    assert int((out[1][0] >= 0).sum()) > 10 * 32  # (the lists are not empty)
