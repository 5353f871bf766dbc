"""Cells over float vectors (``IvfFlatGpuIndex``, ``annlite_ivf_flat_search_topk``): the reference's
``AnnLite(n_cells > 1)`` without ``n_subvectors`` (annlite/index.py:458-466, container.py:88-144), with ``n_probe < n_cells``.

Yardstick, from what the project already had: per query the offsets whose ``_cell_of`` is one of ``idx.probe_cells(q_pre, P)[b]``,
ascending, padded with -1 -> ``ops.rerank_topk(metric, q_pre, idx._vectors, cand, k, valid_bits, sqrt)``.  Ids by ``array_equal``,
distances by their bits; no tolerance, no query left out.  The ``VQCodec`` carries a hand-set codebook (corners of a cube), so
the cells' sizes are the test's choice and not k-means'."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _centroids(C, D):
    """corners of a cube of edge 6 in the first min(D, 3) coordinates, shifted off the origin: rows drawn at a corner + 0.3 N(0, 1)
    lie ten sigma inside their cell"""
    c = np.zeros((C, D), np.float32)
    for j in range(min(D, 3)):
        c[:, j] = 6.0 * ((np.arange(C) >> j) & 1) + 1.0
    assert len({tuple(r) for r in c.tolist()}) == C
    return c


def _vq(C, D, metric):
    from annlite_amd.core.codec.vq import VQCodec
    from annlite_amd.enums import Metric

    vq = VQCodec(C, metric=Metric(metric))
    vq._codebook = _centroids(C, D)
    vq._is_trained = True
    return vq


def _rows(rs, sizes, D, noise=0.3):
    """(x, cell of every row): sizes[c] rows around centroid c, shuffled so that a cell's offsets are scattered"""
    cent = _centroids(len(sizes), D)
    cell = rs.permutation(np.repeat(np.arange(len(sizes)), sizes))
    x = (cent[cell] + noise * rs.randn(len(cell), D)).astype(np.float32)
    return x, cell


def _queries(rs, C, D, B, noise=0.5):
    cent = _centroids(C, D)
    return (cent[rs.randint(0, C, size=B)] + noise * rs.randn(B, D)).astype(np.float32)


def _index(metric, D, vq, x, ids=None, n_probe=None, **kw):
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex
    from annlite_amd.enums import Metric

    idx = IvfFlatGpuIndex(D, vq_codec=vq, n_probe=n_probe, metric=Metric(metric), initial_size=max(len(x), 1), **kw)
    idx.add_with_ids(x, np.arange(len(x)) if ids is None else ids)
    return idx


def _probed(idx, q, P):
    """(q_pre, cand i64 [B, R]): every query's probed offsets ascending, -1 behind them"""
    import torch

    qd = idx._pre(q)
    cells = idx.probe_cells(qd, P).to(torch.int64)
    N = idx._n_rows
    cell_of = idx._cell_of[:N].to(torch.int64)
    member = torch.zeros((qd.shape[0], N), dtype=torch.bool, device=qd.device)
    for p in range(P):
        member |= cell_of[None, :] == cells[:, p:p + 1]
    rows = torch.arange(N, device=qd.device, dtype=torch.int64)[None, :]
    srt = torch.sort(torch.where(member, rows, torch.full_like(rows, N)), dim=1).values
    R = max(int(member.sum(dim=1).max().item()), 1)
    cand = srt[:, :R]
    return qd, torch.where(cand == N, torch.full_like(cand, -1), cand).contiguous(), cells


def _yardstick(ops, idx, q, k, P, bits=None, probed=None):
    import torch
    from annlite_amd.enums import Metric

    qd, cand, _ = probed or _probed(idx, q, P)
    d, i = ops.rerank_topk(int(idx.metric), qd, idx._vectors, cand, k, valid_bits=idx._valid if bits is None else bits,
                           sqrt=idx.metric == Metric.EUCLIDEAN)
    torch.cuda.synchronize()
    return d.cpu().numpy(), i.cpu().numpy()


def _same(got, want, what):
    (gd, gi), (wd, wi) = got, want
    assert gi.dtype == np.int64 and gd.dtype == np.float32
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:5], gi[gi != wi][:5], wi[gi != wi][:5])
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (what, 'distance bits')


# an empty cell, a cell of one row, a cell of 129 rows (two row tiles, the second nearly empty), cells above 4096 rows (the filter
# runs whatever P is: the largest cell alone exceeds the first sample)
SIZES = [0, 1, 129, 5000, 6000, 3000, 2500, 3370]


@pytest.mark.parametrize('metric', [1, 2, 3])
@pytest.mark.parametrize('D', [3, 96, 128])
def test_pruned_search_equals_exact_rerank_over_the_probed_rows(ops, metric, D):
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.enums import Metric

    C = len(SIZES)
    rs = np.random.RandomState(100 * D + metric)
    x, cell = _rows(rs, SIZES, D)
    N = len(x)
    dup = np.flatnonzero(cell == 4)[:12]
    x[dup] = x[dup[0]]  # ties inside a probed cell: the lower id first
    idx = _index(metric, D, _vq(C, D, metric), x)
    assert np.array_equal(idx._cell_of[:N].cpu().numpy(), cell)  # the cells are the ones this test laid out
    qs = {B: _queries(rs, C, D, B) for B in (1, 5, 300)}
    qs[5][2] = x[dup[3]]               # a query equal to a stored (and duplicated) row
    qs[300][7] = x[np.flatnonzero(cell == 1)[0]]  # ... and to the only row of its cell
    for P in (1, 3, C - 1):
        assert ops.ivf_flat_stages(sum(sorted(SIZES)[-P:]))  # (not the exact-only route)
        for B, q in qs.items():
            probed = _probed(idx, q, P)
            if metric == 1 and B == 300:  # every cell is somebody's nearest: the empty, the one-row and the 129-row cell are probed
                assert len(np.unique(probed[2][:, 0].cpu().numpy())) == C
            for k in (1, 10, 64):
                got = idx.search_batch(q, limit=k, n_probe=P)
                _same(got, _yardstick(ops, idx, q, k, P, probed=probed), (P, B, k))
            assert idx.last_overflowed == 0
        if metric == 1:
            got = idx.search_batch(qs[5], limit=12, n_probe=P)
            assert got[0][2, 0] == 0.0 and np.array_equal(got[1][2], np.sort(dup))  # self-match at exactly 0, its duplicates by id
            got = idx.search_batch(qs[300], limit=1, n_probe=P)
            assert got[0][7, 0] == 0.0 and cell[got[1][7, 0]] == 1
    # every cell visited (P >= C, n_probe=None: what the reference always does) is FlatGpuIndex.search_batch on the same rows
    flat = FlatGpuIndex(D, metric=Metric(metric), initial_size=N)
    flat.add_with_ids(x, np.arange(N))
    for B, k in ((5, 10), (300, 64)):
        want = flat.search_batch(qs[B], limit=k)
        _same(idx.search_batch(qs[B], limit=k), want, ('n_probe=None', B, k))
        _same(idx.search_batch(qs[B], limit=k, n_probe=C), want, ('n_probe=C', B, k))
        _same(idx.search_batch(qs[B], limit=k, n_probe=C + 5), want, ('n_probe>C', B, k))


def test_two_query_tiles_in_one_cell(ops):
    rs = np.random.RandomState(3)
    D, C = 32, 2
    x, cell = _rows(rs, [5000, 4500], D)
    idx = _index(1, D, _vq(C, D, 1), x, n_probe=1)
    q = _queries(rs, C, D, 300)
    q[:200] = (_centroids(C, D)[0] + 0.5 * rs.randn(200, D)).astype(np.float32)  # 200 queries probe cell 0: two tiles of 128 slots
    probed = _probed(idx, q, 1)
    assert int((probed[2][:, 0] == 0).sum().item()) > 128
    for k in (10, 64):
        _same(idx.search_batch(q, limit=k), _yardstick(ops, idx, q, k, 1, probed=probed), k)


def test_several_filter_stages_and_no_overflow(ops):
    """N = 300 000 in four cells, two probed: 150 000 probed rows, more than 32 x 4096, so the filter runs in two stages.  i.i.d.
    normal data: lists of a few hundred entries (320 +- 101 at a growth of 32) against a capacity of 4096."""
    rs = np.random.RandomState(5)
    N, D, C, P, B = 300_000, 16, 4, 2, 64
    x = rs.randn(N, D).astype(np.float32)
    q = rs.randn(B, D).astype(np.float32)
    vq = _vq(C, D, 1)
    vq._codebook = np.zeros((C, D), np.float32)
    vq._codebook[:, 0] = [1, 1, -1, -1]  # the quadrants of the first two coordinates: four cells of about N / 4 rows
    vq._codebook[:, 1] = [1, -1, 1, -1]
    idx = _index(1, D, vq, x, n_probe=P)
    idx._seal()
    strides = ops.ivf_flat_stages(int(idx._sizes_cum[P - 1]))
    assert int(idx._sizes_cum[P - 1]) > 32 * 4096 and len(strides) >= 3, strides  # the first sample + at least two filter stages
    got10 = idx.search_batch(q, limit=10)
    assert idx.last_overflowed == 0
    got64 = idx.search_batch(q, limit=64)
    sub = np.arange(0, B, 4)  # 16 of the queries
    probed = _probed(idx, q[sub], P)
    _same((got10[0][sub], got10[1][sub]), _yardstick(ops, idx, q[sub], 10, P, probed=probed), 'k=10')
    _same((got64[0][sub], got64[1][sub]), _yardstick(ops, idx, q[sub], 64, P, probed=probed), 'k=64')


@pytest.fixture(scope='module')
def small(ops):
    """(index, x, cell, queries): EUCLIDEAN, D = 32, six cells -- shared by the tests below that do not change it"""
    rs = np.random.RandomState(11)
    D, sizes = 32, [4500, 3000, 2000, 40, 5, 0]
    x, cell = _rows(rs, sizes, D)
    idx = _index(1, D, _vq(len(sizes), D, 1), x, n_probe=2)
    return idx, x, cell, _queries(rs, len(sizes), D, 40)


def test_deletes_indices_updates_and_later_adds(ops):
    rs = np.random.RandomState(13)
    D, sizes = 32, [4500, 3000, 2000, 400, 100]
    C, P = len(sizes), 2
    x, cell = _rows(rs, sizes, D)
    N = len(x)
    idx = _index(1, D, _vq(C, D, 1), x, n_probe=P, expand_step_size=1024)
    q = _queries(rs, C, D, 150)
    # a third of the rows, among them EVERY row of cell 1 (which queries probe)
    dead = np.union1d(np.flatnonzero(cell == 1), rs.choice(N, size=N // 3 - sizes[1], replace=False))
    idx.delete(dead.tolist())
    assert idx.size == N - len(dead)
    probed = _probed(idx, q, P)
    assert bool((probed[2] == 1).any())
    for k in (10, 64):
        got = idx.search_batch(q, limit=k)
        _same(got, _yardstick(ops, idx, q, k, P, probed=probed), ('deleted', k))
        assert not np.isin(got[1], dead).any()
    # indices=
    keep = rs.choice(N, size=N // 5, replace=False)
    bits = idx._filter_bits(keep)
    got = idx.search_batch(q, limit=16, indices=keep)
    _same(got, _yardstick(ops, idx, q, 16, P, bits=bits, probed=probed), 'indices')
    assert np.isin(got[1][got[1] >= 0], np.setdiff1d(keep, dead)).all()
    # fewer than k rows in the probed cells: (+inf, -1) padding
    two = np.setdiff1d(np.flatnonzero(cell == 0), dead)[:2].tolist()
    q0 = (_centroids(C, D)[0] + 0.5 * rs.randn(3, D)).astype(np.float32)  # (they probe cell 0)
    got = idx.search_batch(q0, limit=20, indices=two)
    assert (got[1][:, 2:] == -1).all() and np.isinf(got[0][:, 2:]).all() and (np.sort(got[1][:, :2], axis=1) == two).all()
    _same(got, _yardstick(ops, idx, q0, 20, P, bits=idx._filter_bits(two)), 'few')
    # a later add (the store grows, the seal is rebuilt): rows into cell 1 again, under new ids
    more = (_centroids(C, D)[1] + 0.3 * rs.randn(700, D)).astype(np.float32)
    idx.add_with_ids(more, np.arange(N, N + 700))
    assert idx.capacity >= N + 700 and idx.size == N - len(dead) + 700
    got = idx.search_batch(q, limit=10)
    _same(got, _yardstick(ops, idx, q, 10, P), 'added')
    assert (got[1] >= N).any()
    # update_with_ids with a vector of ANOTHER cell: the row moves (row a of cell 0 becomes a row at centroid 3)
    a = int(np.setdiff1d(np.flatnonzero(cell == 0), dead)[0])
    moved = (_centroids(C, D)[3] + 0.01 * rs.randn(D)).astype(np.float32)
    idx.update_with_ids(moved[None, :], [a])
    assert int(idx._cell_of[a].item()) == 3 and idx.size == N - len(dead) + 700
    d, i = idx.search_batch(moved[None, :], limit=1, n_probe=1)
    assert i[0, 0] == a and d[0, 0] == 0.0
    _same(idx.search_batch(q, limit=10), _yardstick(ops, idx, q, 10, P), 'updated')


def test_overflowed_lists_take_the_probed_rows_route(ops):
    """A probed cell of 6000 identical rows: every row ties, the list (4096) overflows, the query is answered by exact sums over
    its probed rows -- the 6000's lowest ids -- and counted."""
    rs = np.random.RandomState(17)
    D, C = 32, 2
    cent = _centroids(C, D)
    x = np.concatenate([np.repeat(cent[0][None, :], 6000, axis=0), (cent[1] + 0.3 * rs.randn(3000, D)).astype(np.float32)])
    ids = rs.permutation(len(x))
    idx = _index(1, D, _vq(C, D, 1), x, ids=ids, n_probe=1)
    q = _queries(rs, C, D, 50)
    probed = _probed(idx, q, 1)
    in0 = (probed[2][:, 0] == 0).cpu().numpy()
    assert 0 < in0.sum() < len(q)
    got = idx.search_batch(q, limit=10)
    assert idx.last_overflowed == int(in0.sum())
    _same(got, _yardstick(ops, idx, q, 10, 1, probed=probed), 'ties')
    assert (got[1][in0] == np.sort(ids[:6000])[:10]).all()


@pytest.mark.parametrize('metric', [1, 2])
def test_non_finite_queries(ops, metric):
    rs = np.random.RandomState(19)
    D, sizes = 32, [4500, 3000, 2000, 40]
    x, _ = _rows(rs, sizes, D)
    idx = _index(metric, D, _vq(len(sizes), D, metric), x, n_probe=2)
    q = _queries(rs, len(sizes), D, 9)
    q[1, 3] = np.inf
    q[2, 0] = -np.inf
    q[4, :] = np.nan
    q[6, 10] = np.nan
    for k in (10, 64):
        _same(idx.search_batch(q, limit=k), _yardstick(ops, idx, q, k, 2), k)  # (for the cells the selection returned)


def test_large_k_device_tensors_and_the_reference_signature(ops, small):
    import torch

    idx, x, cell, q = small
    P = 2
    qd, cand, _ = _probed(idx, q, P)
    # k = 100: the keyed top-k over the probed rows
    d, i = idx.search_batch(q, limit=100)
    wd, wi = idx._keyed_topk(qd, cand, cand >= 0, 100)
    _same((d, i), (torch.sqrt(wd).cpu().numpy(), wi.cpu().numpy()), 'k=100')
    _same((d[:, :64], i[:, :64]), _yardstick(ops, idx, q, 64, P), 'k=100 against k=64')
    # device tensors in, device tensors out
    d, i = idx.search_batch(ops.to_dev(q), limit=10)
    assert isinstance(d, torch.Tensor) and d.is_cuda and i.is_cuda
    _same((d.cpu().numpy(), i.cpu().numpy()), _yardstick(ops, idx, q, 10, P), 'device in')
    # one query, the reference's signature: valid entries only
    d1, i1 = idx.search(q[0], limit=10)
    n0 = min(10, int((cand[0] >= 0).sum().item()))  # (its two cells may be the small ones)
    assert len(d1) == len(i1) == n0 and (i1 >= 0).all() and n0 >= 1


def test_dump_load_round_trip(ops, small, tmp_path):
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex

    idx, x, cell, q = small
    f = tmp_path / 'cells.idx'
    idx.dump(f)
    again = IvfFlatGpuIndex(idx.dim, vq_codec=idx.vq_codec, n_probe=2, metric=idx.metric, index_file=f)
    assert again.size == idx.size and np.array_equal(again._cell_of[:len(x)].cpu().numpy(), cell)
    for k in (10, 64):
        _same(again.search_batch(q, limit=k), idx.search_batch(q, limit=k), k)
    # a flat snapshot and a cells snapshot do not load into each other
    flat = FlatGpuIndex(idx.dim, metric=idx.metric, initial_size=64)
    flat.add_with_ids(x[:50], np.arange(50))
    flat.dump(tmp_path / 'flat.idx')
    with pytest.raises(AssertionError):
        IvfFlatGpuIndex(idx.dim, vq_codec=idx.vq_codec, metric=idx.metric).load(tmp_path / 'flat.idx')
    with pytest.raises(AssertionError):
        FlatGpuIndex(idx.dim, metric=idx.metric).load(f)


def test_facade(ops, tmp_path):
    from annlite_amd import AnnLite
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex
    from annlite_amd.docarray_compat import Document, DocumentArray

    rs = np.random.RandomState(23)
    N, D, C = 3000, 64, 8
    x, _ = _rows(rs, [N // C] * C, D)
    q = _queries(rs, C, D, 20)
    kw = dict(metric='euclidean', n_cells=C, n_probe=2, ivf_prune=True, data_path=str(tmp_path / 'ann'))
    ann = AnnLite(D, **kw)
    ann._vq_codec.seed, ann._vq_codec.n_init, ann._vq_codec.iter = 2, 1, 10
    assert not ann.is_trained
    ann.train(x)
    assert ann.is_trained and ann._vq_codec_path.exists()  # auto_save: a second facade over the same data_path is trained
    assert AnnLite(D, **kw).is_trained
    ann.index(DocumentArray([Document(id=str(i), embedding=x[i], tags={'g': int(i % 3)}) for i in range(N)]))
    idx = ann.vec_index(0)
    assert isinstance(idx, IvfFlatGpuIndex) and idx.n_probe == 2 and idx.size == N

    def by_index(**kws):
        d, i = idx.search_batch(q, limit=10, **kws)
        return d, i

    def check(a, want, what):
        dists, ids = a.search_numpy(q, limit=10) if what != 'filter' else a.search_numpy(q, filter={'g': {'$eq': 1}}, limit=10)
        _same((np.stack(dists).astype(np.float32), np.stack(ids).astype(np.int64)), want, what)

    want = by_index()
    _same(want, _yardstick(ops, idx, q, 10, 2), 'index level')
    check(ann, want, 'search_numpy')
    docs = DocumentArray([Document(id='q%d' % i, embedding=q[i]) for i in range(len(q))])
    ann.search(docs, limit=10)
    assert [[int(m.id) for m in d.matches] for d in docs] == want[1].tolist()
    assert np.array_equal(np.array([[m.scores['euclidean'].value for m in d.matches] for d in docs], np.float32), want[0])
    check(ann, by_index(indices=np.arange(1, N, 3)), 'filter')
    ann.delete([str(i) for i in range(0, N, 7)])
    want = by_index()
    assert not np.isin(want[1], np.arange(0, N, 7)).any() and ann.index_size == N - len(range(0, N, 7))
    check(ann, want, 'deleted')
    ann.dump()
    again = AnnLite(D, **kw)
    assert again.is_trained and again.index_size == ann.index_size and isinstance(again.vec_index(0), IvfFlatGpuIndex)
    check(again, want, 'reopened')
