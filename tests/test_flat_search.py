"""Exact float32 search (``FlatGpuIndex``, ``annlite_flat_search_topk``) -- the reference's default index,
``AnnLite`` without ``n_subvectors`` (annlite/core/index/flat_index.py:15-39, hnsw/index.py:139-167).

Yardstick: ``ops.rerank_topk(metric, q, vectors, cand = every row id ascending, k, valid_bits, sqrt)`` -- the exact distance and
order this project already had, on tables small enough for a wave per query over every row.  Ids by ``array_equal``, distances
by their bits."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

U = 2.0 ** -24


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _index(metric, D, x, ids=None, **kw):
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.enums import Metric

    idx = FlatGpuIndex(D, metric=Metric(metric), initial_size=max(len(x), 1), **kw)
    idx.add_with_ids(x, np.arange(len(x)) if ids is None else ids)
    return idx


def _yardstick(ops, idx, q, k, bits=None):
    import torch
    from annlite_amd.enums import Metric

    qd = idx._pre(q)
    N = idx._n_rows
    cand = torch.arange(N, dtype=torch.int64, device=qd.device)[None, :].expand(qd.shape[0], N).contiguous()
    d, i = ops.rerank_topk(int(idx.metric), qd, idx._vectors, cand, k, valid_bits=idx._valid if bits is None else bits,
                           sqrt=idx.metric == Metric.EUCLIDEAN)
    torch.cuda.synchronize()
    return d.cpu().numpy(), i.cpu().numpy()


def _same(got, want, what):
    (gd, gi), (wd, wi) = got, want
    assert gi.dtype == np.int64 and gd.dtype == np.float32
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:5], gi[gi != wi][:5], wi[gi != wi][:5])
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (what, 'distance bits')


@pytest.mark.parametrize('metric', [1, 2, 3])
@pytest.mark.parametrize('N', [1, 63, 4097, 50000])
@pytest.mark.parametrize('D', [3, 64, 96, 128, 768])
def test_search_equals_exact_rerank_over_all_rows(ops, metric, D, N):
    rs = np.random.RandomState(1000 * D + N + metric)
    x = rs.randn(N, D).astype(np.float32)
    if N > 40:
        x[20:30] = x[20]  # ties: the lower id first
    idx = _index(metric, D, x)
    qs = {B: rs.randn(B, D).astype(np.float32) for B in (1, 5, 130)}
    qs[5][2] = x[N // 2]  # a query equal to a stored row
    qs[130][7] = x[N - 1]
    for B, q in qs.items():
        for k in (1, 10, 16, 50, 64):
            got = idx.search_batch(q, limit=k)
            _same(got, _yardstick(ops, idx, q, k), (B, k))
            if metric == 1 and k == 1 and B in (5, 130):
                b, row = (2, N // 2) if B == 5 else (7, N - 1)
                assert got[0][b, 0] == 0.0 and np.array_equal(x[got[1][b, 0]], x[row])
    # with deletes
    dead = rs.choice(N, size=N // 3, replace=False)
    idx.delete(dead.tolist())
    assert idx.size == N - len(dead)
    for B, k in ((130, 10), (130, 64), (1, 16)):
        got = idx.search_batch(qs[B], limit=k)
        _same(got, _yardstick(ops, idx, qs[B], k), ('deleted', B, k))
        assert not np.isin(got[1], dead).any()
    # with indices=
    keep = rs.choice(N, size=max(1, N // 5), replace=False)
    bits = idx._filter_bits(keep)
    for B, k in ((5, 16), (130, 50)):
        got = idx.search_batch(qs[B], limit=k, indices=keep)
        _same(got, _yardstick(ops, idx, qs[B], k, bits=bits), ('indices', B, k))
        assert np.isin(got[1][got[1] >= 0], np.setdiff1d(keep, dead)).all()
    # one query, the reference's signature: valid entries only
    d1, i1 = idx.search(qs[1][0], limit=10)
    assert len(d1) == len(i1) == min(10, idx.size) and (i1 >= 0).all()


def test_device_tensors_stay_on_the_device_and_updates_overwrite(ops):
    import torch

    rs = np.random.RandomState(5)
    N, D = 9000, 64
    x = rs.randn(N, D).astype(np.float32)
    idx = _index(1, D, x[:5000], expand_step_size=1024)
    idx.add_with_ids(x[5000:], np.arange(5000, N))  # grows by expand_step_size
    assert idx.size == N and idx.capacity >= N and idx.capacity % 1024 == 0
    q = rs.randn(33, D).astype(np.float32)
    d, i = idx.search_batch(ops.to_dev(q), limit=10)
    assert isinstance(d, torch.Tensor) and d.is_cuda and i.is_cuda
    _same((d.cpu().numpy(), i.cpu().numpy()), _yardstick(ops, idx, q, 10), 'device in')
    idx.update_with_ids(q[:4], [11, 12, 13, 14])  # the rows now ARE the first four queries
    d, i = idx.search_batch(q, limit=3)
    assert np.array_equal(i[:4, 0], [11, 12, 13, 14]) and (d[:4, 0] == 0.0).all() and idx.size == N
    _same((d, i), _yardstick(ops, idx, q, 3), 'updated')
    d, i = idx.search_batch(q[:2], limit=20, indices=[3, 4, 5])  # fewer valid rows than the limit: (+inf, -1) padding
    assert (i[:, 3:] == -1).all() and np.isinf(d[:, 3:]).all() and (i[:, :3] >= 0).all()


def test_large_table_float64_ground_truth_and_no_overflow(ops):
    rs = np.random.RandomState(11)
    N, D, B, k = 200_000, 64, 256, 10
    x = rs.randn(N, D).astype(np.float32)
    q = rs.randn(B, D).astype(np.float32)
    idx = _index(1, D, x)
    d, i = idx.search_batch(q, limit=k)
    assert idx.last_overflowed == 0
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    d2 = (x64 ** 2).sum(1)[None, :] - 2.0 * q64 @ x64.T + (q64 ** 2).sum(1)[:, None]
    order = np.argsort(d2, axis=1, kind='stable')[:, :k + 1]
    top = np.take_along_axis(d2, order, axis=1)
    # the exact kernel's error: |d^ - d| <= gamma(ceil(D/64) + 8) d; a query is decided by the float64
    # ground truth when its 10th / 11th gap is more than that error on both sides
    err = 1.01 * (-(-D // 64) + 8) * U * top[:, k]
    decided = (top[:, k] - top[:, k - 1]) > 2.0 * err
    assert (~decided).mean() <= 0.02
    for b in np.flatnonzero(decided):
        assert set(i[b].tolist()) == set(order[b, :k].tolist()), b
    assert np.allclose(d[decided] ** 2, top[decided, :k], rtol=1e-5, atol=0)
    # k = 64: a stage of growth factor r passes about r k +- r sqrt(k) rows per query (here r = 7: 448); the lists hold 4096
    idx.search_batch(q, limit=64)
    assert idx.last_overflowed == 0


def test_overflowed_lists_take_the_all_rows_route(ops):
    rs = np.random.RandomState(13)
    N, D = 20_000, 64
    x = np.tile(rs.randn(1, D).astype(np.float32), (N, 1))  # every row ties at the bound
    near = [17, 4100, 9999, 19_999]
    q = rs.randn(40, D).astype(np.float32)
    x[near] = q[:4] + 0.01 * rs.randn(4, D).astype(np.float32)
    for metric in (1, 2):
        idx = _index(metric, D, x)
        for k in (1, 10, 64):
            got = idx.search_batch(q, limit=k)
            assert idx.last_overflowed > 0
            _same(got, _yardstick(ops, idx, q, k), (metric, k))
            again = idx.search_batch(q, limit=k)  # (the atomics' order differs from launch to launch; the answer must not)
            assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes()
        if metric == 1:
            got = idx.search_batch(q, limit=10)
            assert got[1][0, 0] == 17 and got[1][1, 0] == 4100


@pytest.mark.parametrize('metric', [1, 2])
def test_non_finite_inputs_keep_the_nan_last_order(ops, metric):
    rs = np.random.RandomState(17)
    D = 64
    for N, k in ((6000, 10), (8, 8), (6000, 64)):
        x = rs.randn(N, D).astype(np.float32)
        x[N // 2, 5] = np.nan  # one stored row with a NaN
        q = rs.randn(9, D).astype(np.float32)
        q[1, 3] = np.inf
        q[2, 0] = -np.inf
        q[4, :] = np.nan
        q[6, 10] = np.nan
        idx = _index(metric, D, x)
        got = idx.search_batch(q, limit=k)
        want = _yardstick(ops, idx, q, k)
        _same(got, want, (N, k))
        if N == 8:  # no row is lost: the NaN row comes last, under its id
            for b in (0, 3, 5):
                assert got[1][b, -1] == N // 2 and np.isnan(got[0][b, -1]) and sorted(got[1][b].tolist()) == list(range(8))
        assert (got[1][4] == np.arange(k)).all() and np.isnan(got[0][4]).all()  # the NaN query: every distance NaN, ids ascending


def test_filter_passes_every_row_within_the_bound(ops):
    """The filter stage alone: with the exact k-th distance as the bound, every row at or below it is in the list -- whatever
    the MFMA chain's rounding -- and the list is not the whole table."""
    import torch

    rs = np.random.RandomState(19)
    N, D, B, k = 30_000, 96, 70, 10
    for metric, x in ((1, 1000.0 + 0.01 * rs.randn(N, D)), (1, rs.randn(N, D)), (2, rs.randn(N, D))):
        x = x.astype(np.float32)
        q = (x[rs.choice(N, B)] + 0.001 * rs.randn(B, D)).astype(np.float32)
        idx = _index(metric, D, x)
        qd = idx._pre(q)
        rows = torch.arange(N, dtype=torch.int64, device=qd.device)[None, :].expand(B, N).contiguous()
        exact = ops.exact_gather_dist(metric, qd, idx._vectors, rows)
        bound = torch.sort(exact, dim=1).values[:, k - 1].contiguous()
        cand, count = ops.flat_filter(metric, qd, idx._vectors, idx._norms, bound, valid_bits=idx._valid, n_rows=N)
        torch.cuda.synchronize()
        cand, count, exact, bound = cand.cpu().numpy(), count.cpu().numpy(), exact.cpu().numpy(), bound.cpu().numpy()
        cap = ops.flat_list_capacity()
        for b in range(B):
            must = np.flatnonzero(exact[b] <= bound[b])
            assert len(must) >= k
            if count[b] <= cap:
                lst = cand[b, :count[b]]
                assert len(set(lst.tolist())) == len(lst) and np.isin(must, lst).all(), (metric, b)
        if x.mean() < 1.0:  # (rows far apart relative to their norms: the slack lets few extra rows in)
            assert (count <= 4 * k).all()
        # a NaN / infinite bound passes everything: the list overflows
        bad = torch.full_like(torch.from_numpy(bound), float('nan')).to(qd.device)
        bad[::2] = float('inf')
        _, count = ops.flat_filter(metric, qd, idx._vectors, idx._norms, bad, valid_bits=idx._valid, n_rows=N)
        assert (count.cpu().numpy() > cap).all()


def test_strided_stages_bit_equal_and_strided_filter_addressing(ops):
    """N large enough for a filter stage over every stride-th row (N > 32 x 4096), against the yardstick bit for bit; and the filter
    alone with a stride: its candidates are table row ids of the strided set, and every strided row within the bound is among them."""
    import torch

    rs = np.random.RandomState(31)
    N, D, B = 150_001, 64, 130
    x = rs.randn(N, D).astype(np.float32)
    x[70_000:70_010] = x[70_000]
    q = rs.randn(B, D).astype(np.float32)
    q[3] = x[70_003]
    for metric in (1, 2):
        idx = _index(metric, D, x)
        idx.delete(list(range(5, N, 11)))
        for k in (10, 64):
            _same(idx.search_batch(q, limit=k), _yardstick(ops, idx, q, k), (metric, k))
            assert idx.last_overflowed == 0
        qd = idx._pre(q)
        for stride in (7, 36):
            rows = torch.arange(0, N, stride, dtype=torch.int64, device=qd.device)
            exact = ops.exact_gather_dist(metric, qd, idx._vectors, rows[None, :].expand(B, -1).contiguous())
            ok = idx._valid_bool[rows]
            exact = torch.where(ok[None, :], exact, torch.full_like(exact, float('inf')))
            bound = torch.sort(exact, dim=1).values[:, 19].contiguous()
            cand, count = ops.flat_filter(metric, qd, idx._vectors, idx._norms, bound, valid_bits=idx._valid, n_rows=N, stride=stride)
            torch.cuda.synchronize()
            cand, count, exact, bound, rows_h = cand.cpu().numpy(), count.cpu().numpy(), exact.cpu().numpy(), bound.cpu().numpy(), rows.cpu().numpy()
            assert (count >= 20).all() and (count <= 200).all()
            for b in range(B):
                lst = cand[b, :count[b]]
                assert (lst % stride == 0).all() and (lst < N).all() and len(set(lst.tolist())) == len(lst)
                assert np.isin(rows_h[exact[b] <= bound[b]], lst).all(), (metric, stride, b)


def test_non_finite_inputs_beyond_64(ops):
    """limit > 64 with inf / NaN queries and a NaN row: the (distance, id) order of all exact distances, NaN last, (+inf, -1) for
    +inf distances only (-inf keeps its id) -- what the k <= 64 path returns in its first 64 places."""
    import torch

    rs = np.random.RandomState(37)
    N, D = 9000, 64
    x = rs.randn(N, D).astype(np.float32)
    x[4500, 5] = np.nan
    q = rs.randn(9, D).astype(np.float32)
    q[1, 3] = np.inf
    q[2, 0] = -np.inf
    q[4, :] = np.nan
    for metric in (1, 2):
        idx = _index(metric, D, x)
        d, i = idx.search_batch(q, limit=100)
        qd = idx._pre(q)
        rows = torch.arange(N, dtype=torch.int64, device=qd.device)
        exact = ops.exact_gather_dist(metric, qd, idx._vectors, rows[None, :].expand(9, N).contiguous()).cpu().numpy()
        for b in range(9):
            nan = np.isnan(exact[b])
            order = np.lexsort((np.arange(N), np.where(nan, np.float32(0), exact[b]), nan))[:100]
            wd = exact[b][order]
            wi = np.where(wd == np.inf, -1, order)
            with np.errstate(invalid='ignore'):
                wd = np.sqrt(wd) if metric == 1 else wd
            assert np.array_equal(i[b], wi), (metric, b)
            assert np.array_equal(np.isnan(d[b]), np.isnan(wd)) and np.array_equal(d[b][~np.isnan(wd)], wd[~np.isnan(wd)]), (metric, b)
        d64, i64 = idx.search_batch(q, limit=64)
        assert np.array_equal(i64, i[:, :64]) and np.array_equal(d64.view(np.uint32), d[:, :64].view(np.uint32))


def test_overflow_counter_belongs_to_the_last_search(ops):
    rs = np.random.RandomState(41)
    N, D = 20_000, 64
    x = np.tile(rs.randn(1, D).astype(np.float32), (N, 1))
    q = rs.randn(8, D).astype(np.float32)
    idx = _index(1, D, x)
    idx.search_batch(q, limit=10)
    assert idx.last_overflowed == 8
    idx.search_batch(q[:0], limit=10)  # an empty batch ran no filter: nothing overflowed
    assert idx.last_overflowed == 0
    idx.search_batch(q, limit=10)
    assert idx.last_overflowed == 8
    d, i = idx.search_batch(q, limit=100)  # limit > 64 counts its own overflowed lists
    assert idx.last_overflowed == 8 and np.array_equal(i, np.tile(np.arange(100), (8, 1)))
    y = rs.randn(N, D).astype(np.float32)
    idx.update_with_ids(y, np.arange(N))
    idx.search_batch(q, limit=100)
    assert idx.last_overflowed == 0


def test_limit_above_64(ops):
    import torch

    rs = np.random.RandomState(23)
    N, D, B = 20_000, 128, 19
    x = rs.randn(N, D).astype(np.float32)
    x[50:60] = x[50]
    q = rs.randn(B, D).astype(np.float32)
    for metric in (1, 3):
        idx = _index(metric, D, x)
        idx.delete(list(range(0, N, 7)))
        d, i = idx.search_batch(q, limit=100)
        qd = idx._pre(q)
        rows = torch.arange(N, dtype=torch.int64, device=qd.device)
        exact = ops.exact_gather_dist(metric, qd, idx._vectors, rows[None, :].expand(B, N).contiguous())
        exact[:, ::7] = float('inf')
        sd, si = torch.sort(exact, dim=1, stable=True)
        sd = torch.sqrt(sd[:, :100]) if metric == 1 else sd[:, :100]
        _same((d, i), (sd.cpu().numpy(), si[:, :100].cpu().numpy()), metric)
        d64, i64 = idx.search_batch(q, limit=64)
        assert np.array_equal(i64, i[:, :64]) and np.array_equal(d64.view(np.uint32), d[:, :64].view(np.uint32))
    small = _index(1, D, x[:70])
    d, i = small.search_batch(q, limit=100)  # more than the table holds: (+inf, -1) padding
    assert (i[:, 70:] == -1).all() and np.isinf(d[:, 70:]).all() and (np.sort(i[:, :70], axis=1) == np.arange(70)).all()


def test_facade_round_trip(ops, tmp_path):
    from annlite_amd import AnnLite
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.index import Document, DocumentArray

    rs = np.random.RandomState(29)
    N, D = 7000, 64
    x = rs.randn(N, D).astype(np.float32)
    q = rs.randn(6, D).astype(np.float32)
    q[0] = x[123]
    ann = AnnLite(D, metric='euclidean', data_path=tmp_path, columns=[('parity', int)])
    assert isinstance(ann.vec_index(0), FlatGpuIndex) and ann.is_trained
    ann.index(DocumentArray([Document(id=str(n), embedding=x[n], tags={'parity': n % 2}) for n in range(N)]))
    assert ann.stat['total_docs'] == N and ann.index_size == N
    d, ids = ann.search_numpy(q, limit=10)
    brute = np.sqrt(((x[None, :, :].astype(np.float64) - q[:, None, :]) ** 2).sum(2))
    for b in range(6):
        assert np.array_equal(ids[b], np.argsort(brute[b], kind='stable')[:10]) and np.allclose(d[b], np.sort(brute[b])[:10], rtol=1e-5)
    assert d[0][0] == 0.0 and ids[0][0] == 123
    qd = DocumentArray([Document(id='q%d' % b, embedding=q[b]) for b in range(6)])
    ann.search(qd, limit=5)
    assert [m.id for m in qd[0].matches] == [str(v) for v in ids[0][:5]]
    assert qd[0].matches[0].scores['euclidean'].value == 0.0
    fd, fids = ann.search_numpy(q, filter={'parity': {'$eq': 1}}, limit=10)  # through the validity bitmap
    for b in range(6):
        odd = np.flatnonzero(np.arange(N) % 2 == 1)
        assert np.array_equal(fids[b], odd[np.argsort(brute[b][odd], kind='stable')[:10]])
    ann.delete([str(v) for v in ids[1][:3]])
    upd = next(v for v in range(N) if v not in ids[1][:3])
    ann.update(DocumentArray([Document(id=str(upd), embedding=q[2], tags={'parity': 1})]))  # it now IS query 2 (under a fresh offset)
    d2, ids2 = ann.search_numpy(q, limit=10)
    assert not np.isin(ids2[1], ids[1][:3]).any() and ids2[2][0] == upd and d2[2][0] == 0.0
    assert ann.index_size == N - 3
    f2 = ann.search_numpy(q, filter={'parity': {'$eq': 1}}, limit=10)[1]
    ann.dump()
    again = AnnLite(D, metric='euclidean', data_path=tmp_path, columns=[('parity', int)])
    assert again.index_size == N - 3 and again.total_docs == N - 3
    d3, ids3 = again.search_numpy(q, limit=10)
    for b in range(6):
        assert np.array_equal(ids3[b], ids2[b]) and np.array_equal(d3[b].view(np.uint32), d2[b].view(np.uint32))
    f3 = again.search_numpy(q, filter={'parity': {'$eq': 1}}, limit=10)[1]
    # (the updated document carries parity 1 under its even id: the filter goes by the tags)
    assert all(((v % 2 == 1) | (v == upd)).all() for v in f3) and f3[2][0] == upd
    assert all(np.array_equal(a, b) for a, b in zip(f3, f2))
    with pytest.warns(UserWarning):
        AnnLite(D, data_path=tmp_path / 'two', devices=[0, 1])
