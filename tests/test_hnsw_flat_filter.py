"""``HnswFlatGpuIndex(filter_search='graph')`` ("filtered walk"): a search that carries a filter answered on the
graph -- the walk routes through every row, only admitted rows are listed -- against the exact filtered search of ``FlatGpuIndex`` on
the same rows, and through the ``AnnLite`` facade.

The recall bound: the filtered walk's recall@10 against the exact filtered answer is at least the UNFILTERED walk's recall@10 on the
same index and queries minus 0.03.  Over 256 x 10 answers at recall about 0.9 the standard deviation is about 0.006: the margin is
five of them.

The rows are a rank-8 latent plus noise, as in tests/test_hnsw_flat_search.py: on such rows the correlated filter (one coordinate above
a quantile) admits no row among the 256 nearest of a third of the queries.  The routing list converges on the query's neighbourhood
whatever the filter, so the walk's own list held recall 0.83 / 0.88 (EUCLIDEAN / COSINE) there; the index's convergence test (the k-th
row against the distance the walk reached) sends those queries to the exact search, and the test below checks
that it does: the correlated case re-answers some queries, the random ones none."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

N, D, B, K, EF = 20000, 32, 256, 10, 64
MARGIN = 0.03


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _data(rs, D, r=8):
    A = rs.randn(r, D).astype(np.float32)
    return lambda n: (rs.randn(n, r).astype(np.float32) @ A + 0.05 * rs.randn(n, D).astype(np.float32)).astype(np.float32)


def _recall(got, want, k=K):
    return float(np.mean([len(set(got[b][:k]) & set(want[b][:k])) / k for b in range(len(want))]))


class _World:
    pass


_worlds = {}


def _world(ops, metric_name):
    """Rows, queries, the exact index, the graph index (default ``filter_search``), the three filters and the unfiltered walk's
    recall: made once per metric; the tests that delete rows build their own."""
    from annlite_amd import FlatGpuIndex, HnswFlatGpuIndex, Metric

    if metric_name in _worlds:
        return _worlds[metric_name]
    w = _World()
    w.metric = Metric[metric_name]
    rs = np.random.RandomState(41 + len(metric_name))
    gen = _data(rs, D)
    w.x, w.q = gen(N), gen(B)
    w.flat = FlatGpuIndex(D, metric=w.metric, initial_size=N)
    w.flat.add_with_ids(w.x, np.arange(N))
    w.hn = HnswFlatGpuIndex(D, metric=w.metric, initial_size=N, ef_search=EF)
    w.hn.add_with_ids(w.x, np.arange(N))
    w.filters = {'0.5': np.flatnonzero(rs.rand(N) < 0.5), '0.1': np.flatnonzero(rs.rand(N) < 0.1),
                 'correlated': np.flatnonzero(w.x[:, 0] > np.quantile(w.x[:, 0], 0.84))}  # (the rows on one side of the data: s = 0.16)
    _, fi = w.flat.search_batch(w.q, limit=K)
    _, hi = w.hn.search_batch(w.q, limit=K)
    w.unfiltered_recall = _recall(hi, fi)
    _worlds[metric_name] = w
    return w


@pytest.mark.parametrize('which', ['0.5', '0.1', 'correlated'])
@pytest.mark.parametrize('metric_name', ['EUCLIDEAN', 'COSINE'])
def test_filtered_search_on_the_graph(ops, metric_name, which):
    w = _world(ops, metric_name)
    some = w.filters[which]
    d, i = w.hn.search_batch(w.q, limit=K, indices=some, filter_search='graph')
    assert w.hn.last_filter_path == 'graph'
    ed, ei = w.flat.search_batch(w.q, limit=K, indices=some)
    assert d.shape == (B, K) and i.shape == (B, K)
    assert (i >= 0).all() and np.isin(i, some).all()       # admitted (and live: nothing is deleted here), no missing place
    assert all(len(set(r)) == K for r in i)
    assert (np.diff(d, axis=1) >= 0).all()
    for b in range(B):                                     # an id both return carries the same distance bits
        pos = {int(v): j for j, v in enumerate(ei[b])}
        for j, v in enumerate(i[b]):
            if int(v) in pos:
                assert d[b][j].view(np.uint32) == ed[b][pos[int(v)]].view(np.uint32), (b, j)
    rec = _recall(i, ei)
    print(f'{metric_name} filter {which} (s = {some.size / N:.3f}): recall@10 filtered walk {rec:.4f}, unfiltered walk '
          f'{w.unfiltered_recall:.4f}, re-answered {w.hn.last_filter_reanswered}')
    assert rec >= w.unfiltered_recall - MARGIN, (rec, w.unfiltered_recall)
    # the convergence test: at these shares a random filter admits about ef of the routing list's rows, the correlated one often none
    assert (w.hn.last_filter_reanswered > 0) == (which == 'correlated')


def test_default_index_answers_a_filter_exactly(ops):
    w = _world(ops, 'EUCLIDEAN')
    some = w.filters['0.5']
    assert w.hn.filter_search == 'exact'
    d, i = w.hn.search_batch(w.q, limit=K, indices=some)
    assert w.hn.last_filter_path == 'exact' and w.hn.last_filter_reanswered == 0
    ed, ei = w.flat.search_batch(w.q, limit=K, indices=some)
    assert np.array_equal(i, ei) and np.array_equal(d.view(np.uint32), ed.view(np.uint32))
    d, i = w.hn.search_batch(w.q, limit=K, indices=some, filter_search='exact')
    assert w.hn.last_filter_path == 'exact' and np.array_equal(i, ei)


@pytest.mark.parametrize('metric_name', ['EUCLIDEAN', 'COSINE'])
def test_a_filtered_search_on_the_graph_is_complete(ops, metric_name):
    """Fewer admitted rows than k: the exact filtered answer, ids and bits.  200 scattered rows: ten admitted rows per query."""
    w = _world(ops, metric_name)
    rs = np.random.RandomState(5)
    five = rs.choice(N, 5, replace=False)
    d, i = w.hn.search_batch(w.q, limit=K, indices=five, filter_search='graph')
    assert w.hn.last_filter_path == 'graph'
    ed, ei = w.flat.search_batch(w.q, limit=K, indices=five)
    assert np.array_equal(i, ei) and np.array_equal(d.view(np.uint32), ed.view(np.uint32))
    assert ((i >= 0).sum(1) == 5).all()
    few = rs.choice(N, 200, replace=False)
    d, i = w.hn.search_batch(w.q, limit=K, indices=few, filter_search='graph')
    assert w.hn.last_filter_path == 'graph'
    print(f'{metric_name}: 200 admitted rows, re-answered {w.hn.last_filter_reanswered} of {B}')
    assert (i >= 0).all() and np.isin(i, few).all() and all(len(set(r)) == K for r in i)
    assert (np.diff(d, axis=1) >= 0).all()


def test_deleted_rows_route_the_filtered_walk_and_are_never_returned(ops):
    from annlite_amd import FlatGpuIndex, HnswFlatGpuIndex, Metric

    w = _world(ops, 'EUCLIDEAN')
    some = w.filters['0.5']
    flat = FlatGpuIndex(D, metric=Metric.EUCLIDEAN, initial_size=N)
    flat.add_with_ids(w.x, np.arange(N))
    hn = HnswFlatGpuIndex(D, metric=Metric.EUCLIDEAN, initial_size=N, ef_search=EF)
    hn.add_with_ids(w.x, np.arange(N))
    _, before = hn.search_batch(w.q, limit=K, indices=some, filter_search='graph')
    gone = np.unique(before[:, 0])[::2]  # admitted top-1 rows
    assert gone.size > 20
    hn.delete(gone.tolist())
    flat.delete(gone.tolist())
    d, i = hn.search_batch(w.q, limit=K, indices=some, filter_search='graph')
    assert hn.last_filter_path == 'graph'
    assert (i >= 0).all() and np.isin(i, some).all() and not np.isin(i, gone).any()
    assert (np.diff(d, axis=1) >= 0).all()
    _, ei = flat.search_batch(w.q, limit=K, indices=some)
    assert _recall(i, ei) >= w.unfiltered_recall - MARGIN


def test_constructor_keyword_is_a_rule_with_a_selectivity_floor(ops):
    from annlite_amd import HnswFlatGpuIndex, Metric

    F = HnswFlatGpuIndex.FILTER_WALK_MIN_FRACTION
    assert 0 < F <= 0.5
    w = _world(ops, 'EUCLIDEAN')
    n = 4000
    hn = HnswFlatGpuIndex(D, metric=Metric.EUCLIDEAN, initial_size=n, ef_search=EF, filter_search='graph')
    hn.add_with_ids(w.x[:n], np.arange(n))
    assert hn.filter_search == 'graph'
    rs = np.random.RandomState(9)
    above = rs.choice(n, int(round(2 * F * n)), replace=False)
    below = rs.choice(n, int(round(0.5 * F * n)), replace=False)
    d, i = hn.search_batch(w.q[:32], limit=K, indices=above)
    assert hn.last_filter_path == 'graph' and (i >= 0).all() and np.isin(i, above).all()
    d, i = hn.search_batch(w.q[:32], limit=K, indices=below)
    assert hn.last_filter_path == 'exact' and np.isin(i, below).all()
    d, i = hn.search_batch(w.q[:32], limit=K, indices=below, filter_search='graph')  # per call: an order
    assert hn.last_filter_path == 'graph' and (i >= 0).all() and np.isin(i, below).all()
    d, i = hn.search_batch(w.q[:32], limit=K, indices=above, filter_search='exact')
    assert hn.last_filter_path == 'exact'
    d, i = hn.search_batch(w.q[:32], limit=K, indices=np.zeros(0, np.int64))  # nothing admitted: the exact search's empty answer
    assert hn.last_filter_path == 'exact' and (i == -1).all()


def test_filter_search_is_validated():
    from annlite_amd import HnswFlatGpuIndex

    with pytest.raises(ValueError, match='filter_search'):
        HnswFlatGpuIndex(D, filter_search='bogus')


def test_filter_search_is_validated_per_call(ops):
    w = _world(ops, 'EUCLIDEAN')
    with pytest.raises(ValueError, match='filter_search'):
        w.hn.search_batch(w.q[:4], limit=K, indices=w.filters['0.5'], filter_search='bogus')


def test_filtered_walk_through_the_facade(ops, tmp_path):
    from annlite_amd import AnnLite, FlatGpuIndex, HnswFlatGpuIndex
    from annlite_amd.index import Document, DocumentArray

    w = _world(ops, 'EUCLIDEAN')
    n = 6000
    x, q = w.x[:n], w.q  # (all 256 queries: the recall margin is sized for 2560 answers)
    docs = lambda: DocumentArray([Document(id=str(v), embedding=x[v], tags={'parity': v % 2}) for v in range(n)])
    args = dict(metric='euclidean', graph=True, build='gpu', ef_search=EF, columns=[('parity', int)])
    ann = AnnLite(D, data_path=tmp_path / 'g', filter_search='graph', **args)
    plain = AnnLite(D, data_path=tmp_path / 'p', **args)
    assert type(ann.vec_index(0)) is HnswFlatGpuIndex and ann.vec_index(0).filter_search == 'graph'
    assert plain.vec_index(0).filter_search == 'exact'
    ann.index(docs())
    plain.index(docs())
    flt = {'parity': {'$eq': 1}}
    d, ids = ann.search_numpy(q, filter=flt, limit=10)
    assert ann.vec_index(0).last_filter_path == 'graph'
    ed, eids = plain.search_numpy(q, filter=flt, limit=10)  # (answered exactly)
    assert plain.vec_index(0).last_filter_path == 'exact'
    assert all(len(r) == 10 and (np.asarray(r) % 2 == 1).all() and len(set(r)) == 10 for r in ids)
    _, ui = plain.search_numpy(q, limit=10)
    _, xi = plain.vec_index(0).search_exhaustive(q, limit=10)
    unfiltered = _recall(ui, xi)
    rec = _recall(ids, eids)
    print(f'facade: recall@10 filtered walk {rec:.4f}, unfiltered walk {unfiltered:.4f}')
    assert rec >= unfiltered - MARGIN
    qd = DocumentArray([Document(id=f'q{j}', embedding=q[j]) for j in range(8)])
    ann.search(qd, filter=flt, limit=10)
    for j, doc in enumerate(qd):
        assert [int(m.id) for m in doc.matches] == [int(v) for v in ids[j]]
    # the other float indexes take the keyword and are unchanged
    other = AnnLite(D, metric='euclidean', data_path=tmp_path / 'f', filter_search='graph')
    assert type(other.vec_index(0)) is FlatGpuIndex
