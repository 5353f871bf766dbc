"""Exact float search with ``64 < limit <= 1024`` in HIP (``flat_exact_wide_kernel``: a workgroup per query, a buffer of 4096 keys in
LDS; DESIGN.md section 3.6, "limit above 64").

Truth where the arithmetic allows one: coordinates are integers of magnitude <= 8, so with D <= 130 every partial sum of the f32 chain
is an integer below 2^24 and exact, and numpy's int64 distances ranked by (distance, id) are the answer to the bit.  Ids by
``array_equal``, distances by their bits, no tolerance."""
import numpy as np
import pytest

from conftest import has_gpu


def gpu(test):
    return pytest.mark.gpu(pytest.mark.skipif(not has_gpu(), reason='needs a GPU')(test))


KINDS = {'f32': np.float32, 'f16': np.float16, 'i8': np.int8}
B = 5


def _index(D, x, metric=1, kind='f32', **kw):
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.enums import Metric

    if kind == 'i8' and metric != 3:
        kw['int8_scale'] = 1.0
    idx = FlatGpuIndex(D, dtype=KINDS[kind], metric=Metric(metric), initial_size=len(x), **kw)
    idx.add_with_ids(x, np.arange(len(x)))
    return idx


def _integers(seed, N, D):
    rs = np.random.RandomState(seed)
    return rs.randint(-8, 9, size=(N, D)), rs.randint(-8, 9, size=(B, D))


def _truth(metric, x, q, live, k):
    """int64 distances of the ``live`` rows ranked by (distance, id): ``(f32 [B, k], i64 [B, k])``, (+inf, -1) behind them"""
    d = ((x[None, live] - q[:, None]) ** 2).sum(-1) if metric == 1 else 1 - (x[None, live] * q[:, None]).sum(-1)
    wd, wi = np.full((len(q), k), np.inf, np.float32), np.full((len(q), k), -1, np.int64)
    for b in range(len(q)):
        order = np.lexsort((live, d[b]))[:k]
        wd[b, :len(order)], wi[b, :len(order)] = d[b][order], live[order]
    return (np.sqrt(wd) if metric == 1 else wd), wi


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), (what, np.argwhere(got[1] != want[1])[:5])
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), (what, 'distance bits')


def test_integer_world_stays_below_2_to_24():
    x = np.full((1, 130), 8, np.int64)
    assert ((x - -x) ** 2).sum() < 2 ** 24 and 1 + (x * x).sum() < 2 ** 24  # the largest distance of either metric at D = 130


@gpu
@pytest.mark.parametrize('N', [70, 4096, 4097, 8192, 8193, 20000])
@pytest.mark.parametrize('D', [5, 130])
@pytest.mark.parametrize('kind', ['f32', 'f16', 'i8'])
def test_against_integer_truth(kind, D, N):
    import torch
    from annlite_amd import ops

    torch.cuda.set_device(0)
    x, q = _integers(1000 * D + N, N, D)
    idx = _index(D, x.astype(np.float32), kind=kind)
    idx.delete(list(range(0, N, 7)))
    live = np.flatnonzero(np.arange(N) % 7 != 0)
    qd = ops.to_dev(q.astype(np.float32))
    for metric in (1, 2):
        for k in (65, 100, 1024):
            d, i = ops.flat_search_topk_wide(idx._kind.tag, metric, qd, idx._vectors, idx._norms, k, valid_bits=idx._valid, n_rows=N, scale=1.0,
                                             sqrt=metric == 1)
            _same((d.cpu().numpy(), i.cpu().numpy()), _truth(metric, x, q, live, k), (metric, k))


@gpu
def test_identical_rows_overflow_every_list():
    rs = np.random.RandomState(3)
    idx = _index(64, np.tile(rs.randn(1, 64).astype(np.float32), (20000, 1)), large_k='wide')
    d, i = idx.search_batch(rs.randn(B, 64).astype(np.float32), limit=1024)
    assert idx.last_large_k == 'wide' and idx.last_overflowed == B
    assert np.array_equal(i, np.tile(np.arange(1024), (B, 1))) and (d == d[:, :1]).all()


@gpu
@pytest.mark.parametrize('metric', [1, 2, 3])
@pytest.mark.parametrize('kind', ['f32', 'f16', 'i8'])
def test_wide_equals_host(kind, metric):
    rs = np.random.RandomState(37 + metric)
    N, D = 9000, 64
    x = rs.randn(N, D).astype(np.float32)
    x[4500, 5] = np.nan
    q = rs.randn(9, D).astype(np.float32)
    q[1, 3], q[2, 0], q[4, :] = np.inf, -np.inf, np.nan
    idx = _index(D, x, metric=metric, kind=kind)
    third = np.sort(rs.choice(N, N // 3, replace=False))
    for k in (65, 1000):
        for indices in (None, third):
            want = idx.search_batch(q, limit=k, indices=indices, large_k='host')
            assert idx.last_large_k == 'host'
            flt, ovf = idx.last_flat_filter, idx.last_overflowed
            got = idx.search_batch(q, limit=k, indices=indices, large_k='wide')
            assert (idx.last_large_k, idx.last_flat_filter, idx.last_overflowed) == ('wide', flt, ovf)
            _same(got, want, (k, indices is None))
    idx.search_batch(q, limit=1025, large_k='wide')
    assert idx.last_large_k == 'host'
    idx.search_batch(q, limit=64)
    assert idx.last_large_k is None


@gpu
def test_probed_cells_against_integer_truth():
    from annlite_amd.core.codec.vq import VQCodec
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex
    from annlite_amd.enums import Metric

    N, D, k = 3000, 5, 100
    x, q = _integers(11, N, D)
    vq = VQCodec(4, metric=Metric.EUCLIDEAN)
    vq._codebook = np.zeros((4, D), np.float32)
    vq._codebook[:, 0] = [-7, -2, 6, 100]  # three cells of unequal size along the first coordinate and one no row is nearest to
    vq._is_trained = True
    idx = IvfFlatGpuIndex(D, vq_codec=vq, n_probe=2, metric=Metric.EUCLIDEAN, initial_size=N, large_k='wide')
    idx.add_with_ids(x.astype(np.float32), np.arange(N))
    idx.delete(list(range(0, N, 7)))
    cell_of = idx._cell_of[:N].cpu().numpy()
    assert sorted(np.bincount(cell_of, minlength=4))[0] == 0 and len(set(np.bincount(cell_of, minlength=4))) == 4
    got = idx.search_batch(q.astype(np.float32), limit=k)
    assert idx.last_large_k == 'wide'
    cells = idx.probe_cells(idx._pre(q.astype(np.float32)), 2).cpu().numpy()
    for b in range(B):
        live = np.flatnonzero((np.arange(N) % 7 != 0) & np.isin(cell_of, cells[b]))
        _same((got[0][b:b + 1], got[1][b:b + 1]), _truth(1, x, q[b:b + 1], live, k), b)


def test_large_k_is_validated_and_forwarded():
    import torch
    from annlite_amd import AnnLite, ops
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex

    with pytest.raises(ValueError):
        FlatGpuIndex(8, large_k='device')
    assert FlatGpuIndex(8, large_k='host').large_k == 'host'
    assert AnnLite(8, large_k='host')._vec_indexes[0].large_k == 'host'
    x = torch.zeros((4, 8))
    for k in (64, 1025):
        with pytest.raises(AssertionError, match='bad shape'):
            ops.flat_search_topk_wide('f32', 1, x, x, x[:, 0].contiguous(), k)
