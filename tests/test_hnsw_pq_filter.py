"""``HnswPQGpuIndex(filter_search='graph')`` ("filtered walk"): a search that carries a filter answered on the graph
over PQ codes -- the walk routes through every row, only admitted rows are listed, the list is ranked as the unfiltered search ranks its
candidates -- against the exhaustive filtered search of a ``PQFlatGpuIndex`` with the same codec and options, in the three ranking
modes (EUCLIDEAN by ADC sums, EUCLIDEAN with ``rerank=True``, COSINE by the metric's tables), and through the ``AnnLite`` facade.

The recall bound: the filtered walk's recall@10 against the exact filtered answer is at least the UNFILTERED walk's recall@10 on the
same index and queries, p, minus five standard deviations of a recall measured over B x K = 2560 answers, 5 sqrt(p (1 - p) / 2560),
rounded up to a hundredth; p is measured in the run (``_margin``).

The rows are a rank-8 latent plus noise, as in tests/test_hnsw_flat_filter.py: on such rows the correlated filter (one coordinate above
a quantile) admits no row near many of the queries; the routing list converges on the query's neighbourhood whatever the filter, and the
index's convergence test (the sum of the last list entry the answer draws on -- the k-th where the list is ranked by ADC sums, the
whole list where it is re-ranked -- against the sum the walk reached) sends those queries to the exact search.  The test checks that
it does; the random filters' re-answered counts are printed."""
import math

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

N, D, M, B, K, EF = 20000, 32, 8, 256, 10, 64
MODES = {'adc': ('EUCLIDEAN', False), 'rerank': ('EUCLIDEAN', True), 'cosine': ('COSINE', False)}


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


def _margin(p, answers=B * K):
    """five standard deviations of a recall of ``p`` over ``answers`` answers, rounded up to a hundredth"""
    return math.ceil(5 * math.sqrt(p * (1 - p) / answers) * 100 - 1e-9) / 100


def _codec(x, metric):
    from annlite_amd import PQCodec

    codec = PQCodec(dim=D, n_subvectors=M, n_clusters=256, metric=metric, n_init=1)
    codec.seed = 3
    codec.fit(x[:8192], iter=8)
    return codec


class _World:
    pass


_worlds = {}


def _world(ops, mode):
    """Rows, queries, the codec, the exhaustive index, the graph index (default ``filter_search``), the three filters and the unfiltered
    walk's recall: made once per ranking mode; the tests that delete rows or build differently make their own indexes."""
    from annlite_amd import HnswPQGpuIndex, Metric, PQFlatGpuIndex

    if mode in _worlds:
        return _worlds[mode]
    w = _World()
    w.metric, w.rerank = Metric[MODES[mode][0]], MODES[mode][1]
    rs = np.random.RandomState(43 + len(mode))
    gen = _data(rs, D)
    w.x, w.q = gen(N), gen(B)
    w.codec = _codec(w.x, w.metric)
    w.flat = PQFlatGpuIndex(D, pq_codec=w.codec, metric=w.metric, initial_size=N, rerank=w.rerank)
    w.flat.add_with_ids(w.x, np.arange(N))
    w.hn = HnswPQGpuIndex(D, pq_codec=w.codec, metric=w.metric, initial_size=N, ef_search=EF, rerank=w.rerank)
    w.hn.add_with_ids(w.x, np.arange(N))
    assert w.hn.build == 'gpu' and w.hn.expand_width == 2
    w.filters = {'0.5': np.flatnonzero(rs.rand(N) < 0.5), '0.1': np.flatnonzero(rs.rand(N) < 0.1),
                 'correlated': np.flatnonzero(w.x[:, 0] > np.quantile(w.x[:, 0], 0.84))}  # (the rows on one side of the data: s = 0.16)
    _, fi = w.flat.search_batch(w.q, limit=K)
    _, hi = w.hn.search_batch(w.q, limit=K)
    w.unfiltered_recall = _recall(hi, fi)
    w.margin = _margin(w.unfiltered_recall)
    _worlds[mode] = w
    return w


def _assert_admitted_and_ranked(d, i, admitted, b=B):
    assert d.shape == (b, K) and i.shape == (b, K)
    assert (i >= 0).all() and np.isin(i, admitted).all()  # admitted, no missing place
    assert all(len(set(r)) == K for r in i)
    assert (np.diff(d, axis=1) >= 0).all()


def _assert_shared_ids_carry_the_same_bits(d, i, ed, ei):
    for b in range(len(i)):
        pos = {int(v): j for j, v in enumerate(ei[b])}
        for j, v in enumerate(i[b]):
            if int(v) in pos:
                assert d[b][j].view(np.uint32) == ed[b][pos[int(v)]].view(np.uint32), (b, j)


@pytest.mark.parametrize('which', ['0.5', '0.1', 'correlated'])
@pytest.mark.parametrize('mode', list(MODES))
def test_filtered_search_on_the_graph(ops, mode, which):
    """Measured (one MI355X; recall@10 filtered walk / unfiltered walk, margin, queries re-answered of 256):

        adc     0.5: 1.0000 / 0.9996, 0.01, 0     0.1: 1.0000 / 0.9996, 0.01, 0     correlated: 1.0000 / 0.9996, 0.01, 137
        rerank  0.5: 1.0000 / 1.0000, 0.00, 108   0.1: 1.0000 / 1.0000, 0.00, 256   correlated: 1.0000 / 1.0000, 0.00, 198
        cosine  0.5: 0.9953 / 0.9590, 0.02, 120   0.1: 1.0000 / 0.9590, 0.02, 256   correlated: 0.9938 / 0.9590, 0.02, 176

    On this data the unfiltered re-ranked walk finds every one of its 2560 answers, so the formula's margin is 0.00 there: one missed
    answer fails the case.  With the convergence test at the k-th entry in every mode [rerank-correlated] missed one (0.9996): the
    12th nearest admitted row by ADC sum (116.69) of a query whose walk reached 105.50 with the list's 10th sum at 104.58 -- the re-rank
    draws on entries beyond the k-th, and the list is complete only as far as the walk reached.  Hence the depth of the test in the
    re-ranking modes (the whole list), and their re-answered counts: at a share of 0.1, 64 / 0.1 = 640 places would be needed and the
    routing list has 256, so every query goes back to the exact search."""
    w = _world(ops, mode)
    some = w.filters[which]
    d, i = w.hn.search_batch(w.q, limit=K, indices=some, filter_search='graph')
    assert w.hn.last_filter_path == 'graph'
    ed, ei = w.flat.search_batch(w.q, limit=K, indices=some)
    _assert_admitted_and_ranked(d, i, some)
    _assert_shared_ids_carry_the_same_bits(d, i, ed, ei)
    rec = _recall(i, ei)
    print(f'{mode} filter {which} (s = {some.size / N:.3f}): recall@10 filtered walk {rec:.4f}, unfiltered walk '
          f'{w.unfiltered_recall:.4f}, margin {w.margin:.2f}, re-answered {w.hn.last_filter_reanswered}')
    assert rec >= w.unfiltered_recall - w.margin, (rec, w.unfiltered_recall, w.margin)
    if which == 'correlated':  # the convergence test: the filter admits nothing near many of the queries
        assert w.hn.last_filter_reanswered > 0


@pytest.mark.parametrize('mode', list(MODES))
def test_default_index_answers_a_filter_exactly_as_its_parent(ops, mode):
    w = _world(ops, mode)
    some = w.filters['0.5']
    assert w.hn.filter_search == 'exact'
    d, i = w.hn.search_batch(w.q, limit=K, indices=some)
    assert w.hn.last_filter_path == 'exact' and w.hn.last_filter_reanswered == 0
    ed, ei = w.flat.search_batch(w.q, limit=K, indices=some)
    assert np.array_equal(i, ei) and np.array_equal(d.view(np.uint32), ed.view(np.uint32))
    d, i = w.hn.search_batch(w.q, limit=K, indices=some, filter_search='exact')
    assert w.hn.last_filter_path == 'exact' and np.array_equal(i, ei) and np.array_equal(d.view(np.uint32), ed.view(np.uint32))


@pytest.mark.parametrize('mode', list(MODES))
def test_a_filtered_search_on_the_graph_is_complete(ops, mode):
    """Fewer admitted rows than k: the exact filtered answer, ids and bits.  200 scattered rows: ten admitted rows per query."""
    w = _world(ops, mode)
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
    print(f'{mode}: 5 admitted rows, then 200: re-answered {w.hn.last_filter_reanswered} of {B}')
    _assert_admitted_and_ranked(d, i, few)
    _assert_shared_ids_carry_the_same_bits(d, i, *w.flat.search_batch(w.q, limit=K, indices=few))


def test_deleted_rows_route_the_filtered_walk_and_are_never_returned(ops):
    from annlite_amd import HnswPQGpuIndex, PQFlatGpuIndex

    w = _world(ops, 'adc')
    some = w.filters['0.5']
    flat = PQFlatGpuIndex(D, pq_codec=w.codec, metric=w.metric, initial_size=N)
    flat.add_with_ids(w.x, np.arange(N))
    hn = HnswPQGpuIndex(D, pq_codec=w.codec, metric=w.metric, initial_size=N, ef_search=EF)
    hn.add_with_ids(w.x, np.arange(N))
    _, before = hn.search_batch(w.q, limit=K, indices=some, filter_search='graph')
    gone = np.unique(before[:, 0])[::2]  # admitted top-1 rows
    assert gone.size > 20
    hn.delete(gone.tolist())
    flat.delete(gone.tolist())
    d, i = hn.search_batch(w.q, limit=K, indices=some, filter_search='graph')
    assert hn.last_filter_path == 'graph'
    _assert_admitted_and_ranked(d, i, some)
    assert not np.isin(i, gone).any()
    _, ei = flat.search_batch(w.q, limit=K, indices=some)
    assert _recall(i, ei) >= w.unfiltered_recall - w.margin


def test_constructor_keyword_is_a_rule_with_a_selectivity_floor(ops):
    from annlite_amd import HnswPQGpuIndex

    F = HnswPQGpuIndex.FILTER_WALK_MIN_FRACTION
    assert 0 < F <= 1.0
    w = _world(ops, 'adc')
    n = 4000
    hn = HnswPQGpuIndex(D, pq_codec=w.codec, metric=w.metric, initial_size=n, ef_search=EF, filter_search='graph')
    hn.add_with_ids(w.x[:n], np.arange(n))
    assert hn.filter_search == 'graph'
    rs = np.random.RandomState(9)
    above = rs.choice(n, min(n, int(round(2 * F * n))), replace=False)  # (a floor of 1.0: every row)
    below = rs.choice(n, int(round(0.5 * F * n)), replace=False)
    d, i = hn.search_batch(w.q[:32], limit=K, indices=above)
    assert hn.last_filter_path == 'graph'
    _assert_admitted_and_ranked(d, i, above, 32)
    d, i = hn.search_batch(w.q[:32], limit=K, indices=below)
    assert hn.last_filter_path == 'exact' and np.isin(i, below).all()
    d, i = hn.search_batch(w.q[:32], limit=K, indices=below, filter_search='graph')  # per call: an order
    assert hn.last_filter_path == 'graph'
    _assert_admitted_and_ranked(d, i, below, 32)
    d, i = hn.search_batch(w.q[:32], limit=K, indices=above, filter_search='exact')
    assert hn.last_filter_path == 'exact'
    d, i = hn.search_batch(w.q[:32], limit=K, indices=np.zeros(0, np.int64))  # nothing admitted: the exact search's empty answer
    assert hn.last_filter_path == 'exact' and (i == -1).all()


def test_filter_search_is_validated(ops):
    from annlite_amd import HnswPQGpuIndex

    w = _world(ops, 'adc')
    with pytest.raises(ValueError, match='filter_search'):
        HnswPQGpuIndex(D, pq_codec=w.codec, metric=w.metric, filter_search='bogus')
    with pytest.raises(ValueError, match='filter_search'):
        w.hn.search_batch(w.q[:4], limit=K, indices=w.filters['0.5'], filter_search='bogus')


def test_a_host_built_graph_is_walked_with_a_filter_on_the_gpu(ops):
    from annlite_amd import HnswPQGpuIndex, PQFlatGpuIndex

    w = _world(ops, 'adc')
    n = 6000
    flat = PQFlatGpuIndex(D, pq_codec=w.codec, metric=w.metric, initial_size=n)
    flat.add_with_ids(w.x[:n], np.arange(n))
    hn = HnswPQGpuIndex(D, pq_codec=w.codec, metric=w.metric, initial_size=n, ef_search=EF, build='host')
    hn.add_with_ids(w.x[:n], np.arange(n))
    assert hn.build == 'host' and hn.walk == 'gpu'
    some = np.flatnonzero(np.random.RandomState(2).rand(n) < 0.5)
    d, i = hn.search_batch(w.q, limit=K, indices=some, filter_search='graph')
    assert hn.last_filter_path == 'graph'
    ed, ei = flat.search_batch(w.q, limit=K, indices=some)
    _assert_admitted_and_ranked(d, i, some)
    _assert_shared_ids_carry_the_same_bits(d, i, ed, ei)
    _, ui = hn.search_batch(w.q, limit=K)
    _, xi = flat.search_batch(w.q, limit=K)
    p = _recall(ui, xi)
    rec = _recall(i, ei)
    print(f'host-built graph: recall@10 filtered walk {rec:.4f}, unfiltered walk {p:.4f}, re-answered {hn.last_filter_reanswered}')
    assert rec >= p - _margin(p)


def test_a_host_walk_keeps_the_exact_path(ops):
    from annlite_amd import HnswPQGpuIndex, PQFlatGpuIndex

    w = _world(ops, 'adc')
    n = 3000
    flat = PQFlatGpuIndex(D, pq_codec=w.codec, metric=w.metric, initial_size=n)
    flat.add_with_ids(w.x[:n], np.arange(n))
    hn = HnswPQGpuIndex(D, pq_codec=w.codec, metric=w.metric, initial_size=n, ef_search=EF, walk='host', filter_search='graph')
    hn.add_with_ids(w.x[:n], np.arange(n))
    some = np.arange(0, n, 2)
    d, i = hn.search_batch(w.q[:16], limit=K, indices=some, filter_search='graph')
    assert hn.last_filter_path == 'exact'
    ed, ei = flat.search_batch(w.q[:16], limit=K, indices=some)
    assert np.array_equal(i, ei) and np.array_equal(d.view(np.uint32), ed.view(np.uint32))


def test_filtered_walk_through_the_facade(ops, tmp_path):
    from annlite_amd import AnnLite, HnswPQGpuIndex, PQFlatGpuIndex
    from annlite_amd.index import Document, DocumentArray

    w = _world(ops, 'adc')
    n = 6000
    x, q = w.x[:n], w.q  # (all 256 queries: the recall margin is sized for 2560 answers)
    docs = lambda: DocumentArray([Document(id=str(v), embedding=x[v], tags={'parity': v % 2}) for v in range(n)])
    args = dict(metric='euclidean', n_subvectors=M, graph=True, ef_search=EF, columns=[('parity', int)])

    def make(name, **kw):
        ann = AnnLite(D, data_path=tmp_path / name, **args, **kw)
        ann._pq_codec.seed = 1  # same codebooks for both facades
        ann.train(x[:4096])
        ann.index(docs())
        return ann

    ann, plain = make('g', filter_search='graph'), make('p')
    assert type(ann.vec_index(0)) is HnswPQGpuIndex and ann.vec_index(0).filter_search == 'graph'
    assert plain.vec_index(0).filter_search == 'exact'
    flt = {'parity': {'$eq': 1}}
    ann.vec_index(0).FILTER_WALK_MIN_FRACTION = 0.25  # (this instance's rule: half of the rows pass the floor whatever the class's is)
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
    assert rec >= unfiltered - _margin(unfiltered)
    qd = DocumentArray([Document(id=f'q{j}', embedding=q[j]) for j in range(8)])
    ann.search(qd, filter=flt, limit=10)
    for j, doc in enumerate(qd):
        assert [int(m.id) for m in doc.matches] == [int(v) for v in ids[j]]
    # the exhaustive index over PQ codes takes the keyword and is unchanged
    other = AnnLite(D, metric='euclidean', n_subvectors=M, data_path=tmp_path / 'f', filter_search='graph')
    other.train(x[:4096])
    other.index(DocumentArray([Document(id=str(v), embedding=x[v]) for v in range(64)]))
    assert type(other.vec_index(0)) is PQFlatGpuIndex
