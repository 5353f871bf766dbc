"""``HnswFlatGpuIndex`` end to end: a level-0 graph over float vectors, built in batches and walked on the GPU,
against the exact ``FlatGpuIndex`` on the same rows -- recall, the distances' bits, deletes, filters, large k, persistence, growth --
and through the ``AnnLite`` facade."""
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


def _data(rs, D, r=8):
    A = rs.randn(r, D).astype(np.float32)
    return lambda n: (rs.randn(n, r).astype(np.float32) @ A + 0.05 * rs.randn(n, D).astype(np.float32)).astype(np.float32)


def _recall(got, want, k):
    return float(np.mean([len(set(got[b][:k]) & set(want[b][:k])) / k for b in range(len(want))]))


def _well_formed(index, n, rs, max_links):
    lk = index._gg.links[:n].cpu().numpy().view(np.uint32)
    cnt = lk[:, 0]
    assert cnt.max() <= max_links and (n == 1 or cnt.min() >= 1), (cnt.min(), cnt.max())
    for v in rs.randint(0, n, min(n, 300)):
        row = lk[v, 1:1 + cnt[v]]
        assert (row < n).all() and v not in row and len(np.unique(row)) == len(row), v


def _check_index(tmp_path, rs, metric, D, r, steps, make_pq=None, **knobs):
    """Build over ``steps`` insertion calls, then every property the float graph index promises.  ``make_pq``: builds the PQ graph
    index to compare the recall with (where the dimension allows one)."""
    from annlite_amd import FlatGpuIndex, HnswFlatGpuIndex, Metric

    N, B, k = sum(steps), 128, 10
    gen = _data(rs, D, r)
    x = gen(N)
    q = np.concatenate([gen(B - 32), x[rs.choice(N, 32, replace=False)]])  # the last 32 queries are stored rows
    flat = FlatGpuIndex(D, metric=metric, initial_size=N)
    flat.add_with_ids(x, np.arange(N))
    hn = HnswFlatGpuIndex(D, metric=metric, initial_size=steps[0], **knobs)  # (grows: the vector column is re-allocated between calls)
    n = 0
    for s in steps:
        hn.add_with_ids(x[n:n + s], np.arange(n, n + s))
        n += s
    assert hn.size == N and hn._gg.n == N
    _well_formed(hn, N, rs, 2 * hn.max_connection)
    assert hn._gg.links[:N, 0].float().mean().item() > hn.max_connection * 0.75  # (reverse links fill the lists)
    fd, fi = flat.search_batch(q, limit=k)
    hd, hi = hn.search_batch(q, limit=k)
    rec = _recall(hi, fi, k)
    print('recall@10 float graph', rec)
    assert rec >= 0.9, rec
    if make_pq is not None:
        pq = make_pq(x)
        _, pi = pq.search_batch(q, limit=k)
        rec_pq = _recall(pi, fi, k)
        print('recall@10 PQ graph (rerank)', rec_pq)
        assert rec >= rec_pq - 0.02, (rec, rec_pq)
    # ids both indexes return carry equal distance bits; a stored row that finds itself reports exactly 0.0 (EUCLIDEAN)
    found_self = 0
    for b in range(B):
        pos = {int(i): j for j, i in enumerate(fi[b])}
        for j, i in enumerate(hi[b]):
            if int(i) in pos:
                assert hd[b][j].view(np.uint32) == fd[b][pos[int(i)]].view(np.uint32), (b, j)
    for b in range(B - 32, B):
        own = np.flatnonzero((x == q[b]).all(1))
        hit = np.flatnonzero(np.isin(hi[b], own))
        if len(hit):
            found_self += 1
            if metric == Metric.EUCLIDEAN:
                assert (hd[b][hit] == 0.0).all() and not np.signbit(hd[b][hit]).any()
    assert found_self >= 29
    assert (np.diff(hd, axis=1) >= 0).all() and (hi >= 0).all()
    # ef_search per call; the exact search stays available
    assert _recall(hn.search_batch(q, limit=k, ef_search=200)[1], fi, k) >= rec - 0.01
    ed, ei = hn.search_exhaustive(q, limit=k)
    assert np.array_equal(ei, fi) and np.array_equal(ed.view(np.uint32), fd.view(np.uint32))
    # a filter and k beyond the walk's list are answered exactly
    some = rs.choice(N, N // 3, replace=False)
    a, b_ = hn.search_batch(q, limit=k, indices=some), flat.search_batch(q, limit=k, indices=some)
    assert np.array_equal(a[1], b_[1]) and np.array_equal(a[0].view(np.uint32), b_[0].view(np.uint32))
    a, b_ = hn.search_batch(q[:8], limit=300), flat.search_batch(q[:8], limit=300)
    assert np.array_equal(a[1], b_[1]) and np.array_equal(a[0].view(np.uint32), b_[0].view(np.uint32))
    # k above the wave top-k, inside the list
    d100, i100 = hn.search_batch(q[:8], limit=100, ef_search=128)
    assert (i100 >= 0).all() and (np.diff(d100, axis=1) >= 0).all() and all(len(set(r_)) == 100 for r_ in i100)
    assert np.array_equal(i100[:, :k], hn.search_batch(q[:8], limit=k, ef_search=128)[1])
    # deleted rows route the walk but are never returned
    gone = np.unique(hi[:, 0])
    hn.delete(gone.tolist())
    flat.delete(gone.tolist())
    hd2, hi2 = hn.search_batch(q, limit=k)
    assert not np.isin(hi2, gone).any() and (hi2 >= 0).all()
    assert _recall(hi2, flat.search_batch(q, limit=k)[1], k) >= 0.9
    assert hn.size == N - len(gone) and hn._gg.n == N
    # dump / load: the same ids; rows without links are rebuilt
    hn.dump(tmp_path / 'g.idx')
    again = HnswFlatGpuIndex(D, metric=metric, initial_size=N, **knobs)
    again.load(tmp_path / 'g.idx')
    assert again._gg.n == N and np.array_equal(again._gg.links[:N].cpu().numpy(), hn._gg.links[:N].cpu().numpy())
    hd3, hi3 = again.search_batch(q, limit=k)
    assert np.array_equal(hi2, hi3) and np.array_equal(hd2.view(np.uint32), hd3.view(np.uint32))
    flat.dump(tmp_path / 'f.idx')
    rebuilt = HnswFlatGpuIndex(D, metric=metric, initial_size=N, **knobs)
    rebuilt.load(tmp_path / 'f.idx')
    assert rebuilt._gg.n == N and rebuilt.size == N - len(gone)
    assert _recall(rebuilt.search_batch(q, limit=k)[1], flat.search_batch(q, limit=k)[1], k) >= 0.9
    with pytest.raises(AssertionError):
        flat.load(tmp_path / 'g.idx')  # (the flat index does not take the graph's file for its own)
    # later inserts into the loaded index
    more = gen(500)
    again.add_with_ids(more, np.arange(N, N + 500))
    d4, i4 = again.search_batch(more[:64], limit=1)
    assert (i4[:, 0] >= 0).all() and np.mean(i4[:, 0] == np.arange(N, N + 64)) > 0.9  # a point finds itself
    _well_formed(again, N + 500, rs, 2 * again.max_connection)
    # refusals
    with pytest.raises(RuntimeError, match='insertion order'):
        again.add_with_ids(more[:2], [N + 900, N + 901])
    assert again.size == N - len(gone) + 500  # (refused before anything was stored)
    with pytest.raises(RuntimeError, match='in-place'):
        again.update_with_ids(more[:1], [3])
    again.reset()
    assert again._gg is None and again.size == 0
    assert (again.search_batch(q[:2], limit=3)[1] == -1).all()
    return rec


def test_float_graph_against_the_exact_index_and_the_pq_graph(ops, tmp_path):
    """20 000 clustered points in three calls (3000: exact lists; 9000: crosses BRUTE = 8192 inside the call; 8000: walk batches)."""
    from annlite_amd import HnswPQGpuIndex, Metric, PQCodec

    rs = np.random.RandomState(11)
    D = 32

    def make_pq(x):
        codec = PQCodec(dim=D, n_subvectors=8, n_clusters=256, metric=Metric.EUCLIDEAN, n_init=1)
        codec.seed = 3
        codec.fit(x[:8192], iter=8)
        pq = HnswPQGpuIndex(dim=D, metric=Metric.EUCLIDEAN, pq_codec=codec, initial_size=len(x), ef_search=64, rerank=True)
        assert pq.build == 'gpu'
        pq.add_with_ids(x, np.arange(len(x)))
        return pq

    _check_index(tmp_path, rs, Metric.EUCLIDEAN, D, 8, (3000, 9000, 8000), make_pq=make_pq, max_connection=16, ef_construction=200,
                 ef_search=64)


def test_float_graph_small_batches_cosine(ops, tmp_path, monkeypatch):
    """BRUTE = 512, BATCH = 256: a dozen walk batches with 3000 rows of D = 100 (a lane-strided tail), COSINE.  (No PQ graph to
    compare with: no supported number of sub-spaces divides 100.)"""
    from annlite_amd import Metric
    from annlite_amd.core.index.graph_gpu_build import GpuLevel0GraphF32

    monkeypatch.setattr(GpuLevel0GraphF32, 'BRUTE', 512)
    monkeypatch.setattr(GpuLevel0GraphF32, 'BATCH', 256)
    rs = np.random.RandomState(12)
    _check_index(tmp_path, rs, Metric.COSINE, 100, 8, (300, 1500, 1200), max_connection=16, ef_construction=200, ef_search=64)


def test_float_graph_inner_product(ops, tmp_path, monkeypatch):
    """INNER_PRODUCT walks 1 - <q, x> as the reference's space does: negative distances, the largest rows everyone's neighbours."""
    from annlite_amd import FlatGpuIndex, HnswFlatGpuIndex, Metric
    from annlite_amd.core.index.graph_gpu_build import GpuLevel0GraphF32

    monkeypatch.setattr(GpuLevel0GraphF32, 'BRUTE', 1024)
    monkeypatch.setattr(GpuLevel0GraphF32, 'BATCH', 512)
    rs = np.random.RandomState(13)
    N, D, B, k = 4000, 48, 64, 10
    gen = _data(rs, D)
    x, q = gen(N), gen(B)
    flat = FlatGpuIndex(D, metric=Metric.INNER_PRODUCT, initial_size=N)
    flat.add_with_ids(x, np.arange(N))
    hn = HnswFlatGpuIndex(D, metric=Metric.INNER_PRODUCT, initial_size=N, ef_search=128)
    hn.add_with_ids(x, np.arange(N))
    fd, fi = flat.search_batch(q, limit=k)
    hd, hi = hn.search_batch(q, limit=k)
    assert (fd[:, 0] < 0).any()
    _well_formed(hn, N, rs, 32)
    for b in range(B):  # what the walk finds carries the exact index's bits and order
        pos = {int(i): j for j, i in enumerate(fi[b])}
        for j, i in enumerate(hi[b]):
            if int(i) in pos:
                assert hd[b][j].view(np.uint32) == fd[b][pos[int(i)]].view(np.uint32)
    assert (np.diff(hd, axis=1) >= 0).all() and (hi >= 0).all()
    print('recall@10 inner product', _recall(hi, fi, k))


def test_float_graph_grows_point_by_point(ops):
    """1, 1, 2, 17, 1, 1, 1, 300, 1 points: after every step every search returns a real id and the lists stay well formed."""
    from annlite_amd import HnswFlatGpuIndex, Metric

    rs = np.random.RandomState(5)
    D = 32
    x = _data(rs, D, r=4)(400)
    hn = HnswFlatGpuIndex(D, metric=Metric.EUCLIDEAN, initial_size=256, ef_search=32, max_connection=8, ef_construction=40)
    assert (hn.search_batch(x[:2], limit=3)[1] == -1).all()  # empty: the exact index's empty answer
    n = 0
    for step in (1, 1, 2, 17, 1, 1, 1, 300, 1):
        hn.add_with_ids(x[n:n + step], np.arange(n, n + step))
        n += step
        d, i = hn.search_batch(x[:n][-min(n, 20):], limit=1)
        assert (i[:, 0] >= 0).all() and (i[:, 0] < n).all()
        _well_formed(hn, n, rs, 16)
    d, i = hn.search_batch(x[:n], limit=1)
    assert np.mean(i[:, 0] == np.arange(n)) > 0.97 and (d[i[:, 0] == np.arange(n), 0] == 0.0).all()


def test_float_graph_through_the_facade(ops, tmp_path):
    from annlite_amd import AnnLite, HnswFlatGpuIndex
    from annlite_amd.index import Document, DocumentArray

    rs = np.random.RandomState(29)
    N, D, B = 6000, 32, 32
    gen = _data(rs, D)
    x, q = gen(N), gen(B)
    q[0] = x[123]
    docs = lambda: DocumentArray([Document(id=str(v), embedding=x[v], tags={'parity': v % 2}) for v in range(N)])
    args = dict(metric='euclidean', graph=True, build='gpu', ef_search=96, max_connection=16, ef_construction=100, columns=[('parity', int)])
    ann = AnnLite(D, data_path=tmp_path / 'g', **args)
    assert type(ann.vec_index(0)) is HnswFlatGpuIndex and ann.is_trained
    exact = AnnLite(D, metric='euclidean', data_path=tmp_path / 'f', columns=[('parity', int)])
    ann.index(docs())
    exact.index(docs())
    assert ann.stat['total_docs'] == N and ann.index_size == N and ann.vec_index(0)._gg.n == N
    d, ids = ann.search_numpy(q, limit=10)
    ed, eids = exact.search_numpy(q, limit=10)
    assert np.mean([len(set(ids[b]) & set(eids[b])) / 10 for b in range(B)]) >= 0.9
    assert ids[0][0] == 123 and d[0][0] == 0.0
    fd, fids = ann.search_numpy(q, filter={'parity': {'$eq': 1}}, limit=10)  # a filter is answered exactly
    efd, efids = exact.search_numpy(q, filter={'parity': {'$eq': 1}}, limit=10)
    assert all(np.array_equal(a, b) for a, b in zip(fids, efids)) and all(np.array_equal(a, b) for a, b in zip(fd, efd))
    ann.delete([str(v) for v in ids[1][:3]])
    upd = next(v for v in range(N) if v not in ids[1][:3])
    ann.update(DocumentArray([Document(id=str(upd), embedding=q[2], tags={'parity': 1})]))  # delete + a fresh offset: the next id
    d2, ids2 = ann.search_numpy(q, limit=10)
    assert not np.isin(ids2[1], ids[1][:3]).any() and ids2[2][0] == upd and d2[2][0] == 0.0
    assert ann.index_size == N - 3
    ann.dump()
    again = AnnLite(D, data_path=tmp_path / 'g', **args)
    assert again.index_size == N - 3 and again.total_docs == N - 3 and again.vec_index(0)._gg.n == N + 1
    d3, ids3 = again.search_numpy(q, limit=10)
    for b in range(B):
        assert np.array_equal(ids3[b], ids2[b]) and np.array_equal(d3[b].view(np.uint32), d2[b].view(np.uint32))
    with pytest.raises(NotImplementedError, match="build='gpu'"):
        AnnLite(D, data_path=tmp_path / 'g', **{**args, 'build': None})
