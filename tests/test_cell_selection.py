"""``annlite_ivf_select_cells`` (the coarse quantiser's cell selection, ``AnnLite._cell_selection``, annlite/index.py:458-466)
against the oracle's restatement ``pq_oracle.select_cells``: the fp32 ``fma`` chain of ``cell_distances`` ranked in numpy's order
-- distance ascending, cell ascending, NaN behind every number (+inf included).  Bit-exact cells at every shape the kernel's LDS
holds, ties, signed zeros and non-finite queries / centroids; a pruned index fed non-finite queries must probe the oracle's
cells.  The CPU part pins the oracle's own order for the non-finite rows against a float64 ``argsort``."""
import numpy as np
import pytest

from conftest import has_gpu

LDS_BYTES = 160 * 1024  # the selection kernel keeps 4 queries and 4 distance rows: 16 * (D + C) bytes


def _max_cells(D):
    return LDS_BYTES // 16 - D


NONFINITE = ['pos_inf_coordinate', 'neg_inf_coordinate', 'inf_query', 'nan_coordinate', 'nan_query', 'huge_centroids',
             'nan_centroid']


def _nonfinite(case, B=7, D=16, C=40, seed=0):
    """Queries / centroids with one kind of non-finite value; rows 0 and B - 1 stay finite."""
    rs = np.random.RandomState(seed)
    q = rs.randn(B, D).astype(np.float32)
    c = rs.randn(C, D).astype(np.float32)
    if case == 'pos_inf_coordinate':
        q[1, 3] = np.inf
        q[4, D - 1] = np.inf
    elif case == 'neg_inf_coordinate':
        q[2, 0] = -np.inf
        c[6, 0] = 0.0  # 0 * -inf: a NaN distance under the inner product
    elif case == 'inf_query':
        q[3, :] = np.inf
        q[5, :] = -np.inf
    elif case == 'nan_coordinate':
        q[1, 5] = np.nan
    elif case == 'nan_query':
        q[2, :] = np.nan
    elif case == 'huge_centroids':
        c[5, :] = 1e30     # the squared distance overflows for every query (the inner product stays finite)
        c[9, :] = -1e30
        c[11, 2] = 3e19
    elif case == 'nan_centroid':
        c[7, 4] = np.nan
        c[20, :] = np.nan
    return q, c


def _float64_order(q, c, kind):
    """numpy's stable argsort of the float64 distances, rounded to float32 (an overflowing distance is +inf like the fp32 chain's)."""
    q64, c64 = q.astype(np.float64), c.astype(np.float64)
    with np.errstate(all='ignore'):
        if kind == 0:
            d = ((q64[:, None, :] - c64[None]) ** 2).sum(-1)
        else:
            d = -(q64[:, None, :] * c64[None]).sum(-1)
        d = d.astype(np.float32)
    return np.argsort(d, axis=1, kind='stable')


# ------------------------------------------------------------------------------------------- CPU: the oracle's own order
@pytest.mark.parametrize('case', NONFINITE)
@pytest.mark.parametrize('kind', [0, 1])
def test_oracle_orders_non_finite_cells_like_numpy(oracle, case, kind):
    q, c = _nonfinite(case)
    C = c.shape[0]
    with np.errstate(all='ignore'):
        got = oracle.select_cells(q, c, kind, C)
        d = oracle.cell_distances(q, c, kind)
    assert np.array_equal(got, _float64_order(q, c, kind)), case
    assert not np.isfinite(d).all() or (case, kind) == ('huge_centroids', 1)
    # the order the kernel must follow: numbers ascending (-inf first), then +inf cells by cell, then NaN cells by cell
    for b in range(q.shape[0]):
        row = d[b, got[b]]
        n_num = int((~np.isnan(row) & (row != np.inf)).sum())
        n_inf = int((row == np.inf).sum())
        num = row[:n_num]
        assert (num[:-1] <= num[1:]).all()
        assert (row[n_num:n_num + n_inf] == np.inf).all() and np.isnan(row[n_num + n_inf:]).all()
        assert (np.diff(got[b][n_num:n_num + n_inf]) > 0).all() and (np.diff(got[b][n_num + n_inf:]) > 0).all()


# ------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _select(ops, kind, q, c, P):
    return ops.ivf_select_cells(kind, ops.to_dev(q), ops.to_dev(c), P).cpu().numpy()


def _check_rows(cells, C, P):
    """every row: P distinct cells, all in [0, C)"""
    assert cells.shape[1] == P
    assert ((cells >= 0) & (cells < C)).all()
    assert (np.diff(np.sort(cells, axis=1), axis=1) > 0).all(), 'a cell was selected twice'


def _parity_cases():
    Bs = [1, 3, 4, 5, 1023]
    out = []
    for D in [1, 3, 4, 64, 130, 768]:
        for C in [1, 2, 63, 64, 65, 256, 257, 1000, _max_cells(D)]:
            B = Bs[len(out) % len(Bs)]
            if B * C * D > 3_000_000:  # (keeps the oracle's numpy chain short)
                B = 5
            out.append((D, C, B))
    return out


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason='needs an AMD GPU')
@pytest.mark.parametrize('kind', [0, 1])
def test_select_cells_equals_oracle_at_every_shape(ops, oracle, kind):
    for D, C, B in _parity_cases():
        rs = np.random.RandomState(D * 7919 + C * 31 + B + kind)
        q = rs.randn(B, D).astype(np.float32)
        c = rs.randn(C, D).astype(np.float32)
        if C >= 8:
            c[C // 2] = c[1]          # duplicated centroids: equal distances, the lower cell first
            c[C - 1] = c[1]
            c[3] = 0.0                # a zero centroid: distance |q|^2 (L2) or -0 (inner product)
        want = oracle.select_cells(q, c, kind, C)
        for P in sorted({1, min(2, C), min(16, C), C}):
            got = _select(ops, kind, q, c, P)
            _check_rows(got, C, P)
            assert np.array_equal(got, want[:, :P]), (kind, D, C, B, P)


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason='needs an AMD GPU')
@pytest.mark.parametrize('kind', [0, 1])
def test_select_cells_ties_and_signed_zeros(ops, oracle, kind):
    """Exact ties everywhere: integer-valued vectors with many repeats, centroids orthogonal to a query, -0 coordinates.  Equal
    distances (+0 / -0 included) go by cell."""
    rs = np.random.RandomState(5 + kind)
    D, C, B = 8, 300, 9
    c = rs.randint(-1, 2, size=(C, D)).astype(np.float32)
    c[c == 0] = rs.choice([0.0, -0.0], size=int((c == 0).sum())).astype(np.float32)
    q = rs.randint(-1, 2, size=(B, D)).astype(np.float32)
    q[0] = 0.0
    q[1] = -0.0
    q[2] = 0.0
    q[2, 0] = 1.0
    c[10:40, 0] = 0.0          # orthogonal to query 2: inner product exactly zero
    c[40:50] = -0.0
    d = oracle.cell_distances(q, c, kind)
    assert (d == 0).sum() > 10
    want = oracle.select_cells(q, c, kind, C)
    for P in (1, 7, 64, C):
        got = _select(ops, kind, q, c, P)
        _check_rows(got, C, P)
        assert np.array_equal(got, want[:, :P]), (kind, P)


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason='needs an AMD GPU')
@pytest.mark.parametrize('case', NONFINITE)
@pytest.mark.parametrize('kind', [0, 1])
def test_select_cells_non_finite_inputs(ops, oracle, case, kind):
    """+-inf / NaN in queries or centroids, and centroids whose distances overflow: +inf cells in cell order, then NaN cells in
    cell order (numpy's order), never a cell twice."""
    for C, D in ((40, 16), (300, 12)):
        q, c = _nonfinite(case, B=7, D=D, C=C, seed=C)
        with np.errstate(all='ignore'):
            want = oracle.select_cells(q, c, kind, C)
        for P in (1, 3, 16, C - 1, C):
            got = _select(ops, kind, q, c, P)
            _check_rows(got, C, P)
            assert np.array_equal(got, want[:, :P]), (case, kind, C, P)


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason='needs an AMD GPU')
def test_select_cells_refuses_what_the_lds_cannot_hold(ops):
    import torch

    from annlite_amd import _capi

    D = 64
    C = _max_cells(D) + 1
    q = ops.to_dev(np.ones((3, D), np.float32))
    c = ops.to_dev(np.zeros((C, D), np.float32))
    with pytest.raises(AssertionError):
        ops.ivf_select_cells(0, q, c, 4)
    # through the C entry: ANNLITE_ERR_INVALID, and nothing is launched (the output keeps its contents)
    cells = torch.full((3, 4), -7, dtype=torch.int32, device=q.device)
    rc = _capi.lib().annlite_ivf_select_cells(0, q.data_ptr(), 3, D, c.data_ptr(), C, 4, cells.data_ptr(), _capi.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _capi.ERR_INVALID
    assert (cells.cpu().numpy() == -7).all()
    assert ops.ivf_select_cells(0, q, c[:C - 1], 4).shape == (3, 4)  # one cell fewer fits


# ------------------------------------------------------------------------------------------- GPU: end to end
def _pruned_against_oracle(oracle, M, k, metric_name):
    """A pruned index asked with the non-finite queries of the flat scan's tests, and the oracle's pruned search over the cells the
    ORACLE selects (the probes are not taken from the GPU).  Yields (case, queries, GPU result, oracle result, path)."""
    from test_ivf import _build
    from test_round4_gpu import _nonfinite_inputs

    from annlite_amd import Metric, ops

    metric = Metric[metric_name]
    kind = 0 if metric == Metric.EUCLIDEAN else 1
    omet = oracle.EUCLIDEAN if metric == Metric.EUCLIDEAN else oracle.INNER_PRODUCT
    dsub, C, P, N = 4, 16, 5, 6000
    idx, codec, vq, x = _build(N, M * dsub, M, C, metric, seed=M + k)
    codes = ops.codes_to_numpy(idx._plain_codes(idx._n_rows))
    cells_of = idx._cell_of[:idx._n_rows].cpu().numpy()
    for case in ('inf_coordinate', 'inf_query', 'nan_query', 'ip_inf_query'):
        _, _, q, _ = _nonfinite_inputs(case, M, dsub, 100, 21, 256, seed=3)
        d, i = idx.search_batch(q, limit=k, n_probe=P)
        with np.errstate(all='ignore'):
            probe = oracle.select_cells(q, vq.codebook, kind, P)
            od, oi = oracle.ivf_search(q, codec.codebooks, codes, cells_of, probe, omet, k)
        yield case, q, (d, i), (od, oi), probe, cells_of, idx.last_pruned_path


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason='needs an AMD GPU')
@pytest.mark.parametrize('M,k,path', [(16, 10, 'byte-table cell tiles'), (32, 10, 'u16'), (16, 20, 'u16')])
@pytest.mark.parametrize('metric_name', ['EUCLIDEAN', 'INNER_PRODUCT'])
def test_pruned_search_with_non_finite_queries_probes_the_oracle_cells(oracle, M, k, path, metric_name):
    """Byte-table cell tiles: every query equals the oracle bit for bit.  u16 tile scan + re-score: the finite queries do; a query
    whose every distance is +-inf / NaN gets the oracle's distances from rows of the oracle's cells, but not the lowest ids of that
    tie (see the xfail test below)."""
    for case, q, (d, i), (od, oi), probe, cells_of, used in _pruned_against_oracle(oracle, M, k, metric_name):
        assert path in used, used
        fin = np.isfinite(q).all(1) if path == 'u16' else np.ones(q.shape[0], bool)
        assert np.array_equal(oi[fin], i[fin]), (case, metric_name)
        assert np.array_equal(od, d, equal_nan=True), (case, metric_name)
        for b in np.nonzero(~fin)[0]:
            assert len(set(i[b].tolist())) == k and np.isin(cells_of[i[b]], probe[b]).all(), (case, b)


@pytest.mark.gpu
@pytest.mark.skipif(not has_gpu(), reason='needs an AMD GPU')
@pytest.mark.xfail(strict=True, reason='u16 pruned path: rows tied at +-inf / NaN do not come back lowest id first; cause not yet located -- '
                                       'the re-score is excluded (it ties by id on given lists: tests/test_ivf_stage_kernels.py)')
@pytest.mark.parametrize('M,k', [(32, 10), (16, 20)])
def test_pruned_u16_path_degenerate_query_ties_by_id(oracle, M, k):
    for case, q, (d, i), (od, oi), probe, cells_of, used in _pruned_against_oracle(oracle, M, k, 'EUCLIDEAN'):
        assert np.array_equal(oi, i), case
