"""``AnnLite`` with declared ``columns``: a filter that compiles over them is evaluated on the device (``last_filter_eval == 'gpu'``)
and selects the rows ``filter.select`` selects -- so every search, ``filter()`` and ``get_docs()`` answer exactly as the host path.

Two facades hold the same rows: the first indexes the documents and dumps; the second reopens a copy of its files with
``filter_eval='host'`` (the same codecs, the same graph, the same tags -- and its columns refilled from the restored tags)."""
import shutil

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

N, D, NQ = 6000, 32, 16
COLUMNS = [('price', float), ('n', int), ('cat', str)]
CATS = ['red', 'green', 'blue', 'grey', 'black', 'white', 'rose']
FILTERS = [
    {'n': {'$lt': 50}},
    {'price': {'$gte': 10.0, '$lt': 60.5}, 'cat': {'$in': ['red', 'blue', 'rose']}},
    {'$or': {'n': {'$in': [1, 2, 3, 5, 8, 13, 21, 34, 55, 89]}, '$and': {'price': {'$gt': 90}, 'cat': {'$neq': 'grey'}}}},
    {'$not': {'cat': {'$lt': 'g'}}, 'n': {'$gte': 20.5}},
    {'cat': 'black'},
]
NOTHING = {'n': {'$gt': 1000}}
FEW = {'n': 7, 'cat': 'red', 'price': {'$lt': 50}}  # fewer rows than the limit


def _data():
    rs = np.random.RandomState(77)
    x = rs.randn(N, D).astype(np.float32)
    q = rs.randn(NQ, D).astype(np.float32)
    tags = []
    for r in range(N):
        t = {'extra': r % 3}  # (not declared)
        if r % 13 != 5:
            t['price'] = float(rs.randint(0, 400)) / 4 if r % 9 else int(rs.randint(0, 100))
        if r % 17 != 3:
            t['n'] = int(rs.randint(0, 100))
        if r % 11 != 7:
            t['cat'] = CATS[int(rs.randint(len(CATS)))]
        tags.append(t)
    return x, q, tags


@pytest.fixture(scope='module')
def world():
    import torch

    torch.cuda.set_device(0)
    return _data()


def _docs(x, tags, ids=None):
    from annlite_amd.index import Document, DocumentArray

    ids = range(len(x)) if ids is None else ids
    return DocumentArray([Document(id=str(i), embedding=x[j], tags=tags[j]) for j, i in enumerate(ids)])


def _pair(world, tmp_path, train=False, **kw):
    """(the facade that evaluates filters on the device, the one reopened from a copy of its files that keeps the host path)"""
    from annlite_amd import AnnLite

    x, q, tags = world
    dev = AnnLite(D, metric='euclidean', data_path=tmp_path / 'dev', columns=COLUMNS, **kw)
    assert dev.last_filter_eval is None
    if train:
        dev._pq_codec.seed = 1
        if dev._vq_codec is not None:
            dev._vq_codec.seed = 2
        dev.train(x[:4096])
    dev.index(_docs(x, tags))
    dev.search_numpy(q[:1], limit=3)  # (whatever the index builds lazily is built before the dump)
    dev.dump()
    shutil.copytree(tmp_path / 'dev', tmp_path / 'host')
    host = AnnLite(D, metric='euclidean', data_path=tmp_path / 'host', columns=COLUMNS, filter_eval='host', **kw)
    assert host.index_size == dev.index_size == N
    return dev, host


def _same_answers(dev, host, q, filters=FILTERS, limit=10):
    for flt in filters:
        d, i = dev.search_numpy(q, filter=flt, limit=limit)
        assert dev.last_filter_eval == 'gpu', flt
        hd, hi = host.search_numpy(q, filter=flt, limit=limit)
        assert host.last_filter_eval == 'host'
        assert len(i) == len(hi) == len(q)
        for b in range(len(q)):
            assert np.array_equal(i[b], hi[b]) and np.array_equal(np.asarray(d[b]).view(np.uint32), np.asarray(hd[b]).view(np.uint32)), (flt, b)
        assert sum(len(r) for r in i) > 0


def _admitted(tags, flt):
    from annlite_amd.filter import select

    return select(tags, flt)


def test_flat_index_and_the_whole_lifecycle(world, tmp_path):
    from annlite_amd import AnnLite, FlatGpuIndex
    from annlite_amd.columns import RowMask

    x, q, tags = world
    dev, host = _pair(world, tmp_path)
    assert type(dev.vec_index(0)) is FlatGpuIndex
    assert isinstance(dev._filter_offsets(FILTERS[0]), RowMask) and isinstance(host._filter_offsets(FILTERS[0]), np.ndarray)
    _same_answers(dev, host, q)
    # the answer is the filter's rows: ids from the admitted set, in exact order
    d, i = dev.search_numpy(q, filter=FILTERS[1], limit=10)
    adm = np.asarray(_admitted(tags, FILTERS[1]))
    for b in range(NQ):
        dist = ((x[adm].astype(np.float64) - q[b]) ** 2).sum(1)
        assert np.array_equal(i[b], adm[np.argsort(dist, kind='stable')[:10]])
    # nothing selected, and fewer than the limit
    for ann in (dev, host):
        d, i = ann.search_numpy(q, filter=NOTHING, limit=10)
        assert all(len(r) == 0 for r in i) and all(len(r) == 0 for r in d)
        few = _admitted(tags, FEW)
        assert 0 < len(few) < 10
        d, i = ann.search_numpy(q, filter=FEW, limit=10)
        assert all(sorted(r.tolist()) == few for r in i)
    assert dev.last_filter_eval == 'gpu' and host.last_filter_eval == 'host'
    # a field that is not declared: the host answers, the same rows
    for flt in ({'extra': 1}, {'n': {'$lt': 50}, 'extra': {'$neq': 0}}, {'n': np.int64(5)}):
        d, i = dev.search_numpy(q, filter=flt, limit=10)
        assert dev.last_filter_eval == 'host'
        hd, hi = host.search_numpy(q, filter=flt, limit=10)
        assert all(np.array_equal(a, b) for a, b in zip(i, hi)) and all(np.array_equal(a, b) for a, b in zip(d, hd))
    # the same errors, from either path
    for ann in (dev, host):
        with pytest.raises(ValueError, match='not supported'):
            ann.search_numpy(q, filter={'n': {'$like': 3}}, limit=10)
    # filter() / get_docs(): the same documents in the same order, order_by included
    for flt in FILTERS + [NOTHING, FEW, None, {}]:
        for kw in (dict(limit=25), dict(limit=0, order_by='price'), dict(limit=40, offset=7, order_by='n', ascending=False)):
            got, want = dev.filter(flt, **kw), host.filter(flt, **kw)
            assert [m.id for m in got] == [m.id for m in want], (flt, kw)
        assert [m.id for m in dev.get_docs(flt, limit=30, order_by='cat')] == [m.id for m in host.get_docs(flt, limit=30, order_by='cat')]
    assert len(dev.filter(FILTERS[0], limit=0)) == len(_admitted(tags, FILTERS[0]))
    # delete / update
    gone = [str(v) for v in _admitted(tags, FILTERS[0])[:40:2]] + ['31', '32', '33']
    upd = [6, 65, 4000]  # (not among the deleted)
    new_tags = [{'n': 1, 'price': 11.5, 'cat': 'rose'}, {'cat': 'red'}, {'n': 99}]
    for ann in (dev, host):
        ann.delete(gone)
        ann.update(_docs(x[upd] + 0.5, new_tags, ids=upd))
        assert ann.index_size == N - len(set(gone))
    _same_answers(dev, host, q)
    now = [m.id for m in dev.filter(FILTERS[0], limit=0)]
    assert not set(now) & set(gone) and '6' in now and '4000' not in now and now == [m.id for m in host.filter(FILTERS[0], limit=0)]
    # dump -> reopen: the columns are refilled from the restored tags
    dev.dump()
    again = AnnLite(D, metric='euclidean', data_path=tmp_path / 'dev', columns=COLUMNS)
    assert again.index_size == dev.index_size and len(again._columns) == len(dev._columns) == N + 3
    _same_answers(again, host, q)
    # an irregular value added later: filters that name the column go to the host, the others stay
    odd = [{'n': 3.5, 'price': 1.0, 'cat': 'red'}]
    for ann in (again, host):
        ann.index(_docs(x[:1] * 2, odd, ids=['900001']))
    assert again._columns.irregular == {'n'}
    d, i = again.search_numpy(q, filter=FILTERS[0], limit=10)
    assert again.last_filter_eval == 'host'
    hd, hi = host.search_numpy(q, filter=FILTERS[0], limit=10)
    assert all(np.array_equal(a, b) for a, b in zip(i, hi))
    _same_answers(again, host, q, filters=[FILTERS[4], {'price': {'$lt': 2.0}}])
    # clear
    for ann in (again, host):
        ann.clear()
        assert ann.index_size == 0 and all(len(r) == 0 for r in ann.search_numpy(q, filter=FILTERS[0], limit=5)[1])
    assert len(again._columns) == 0 and not again._columns.irregular
    for ann in (again, host):
        ann.index(_docs(x[:300], tags[:300]))
    _same_answers(again, host, q)


def test_pq_scan(world, tmp_path):
    from annlite_amd import PQFlatGpuIndex

    dev, host = _pair(world, tmp_path, train=True, n_subvectors=8)
    assert type(dev.vec_index(0)) is PQFlatGpuIndex
    _same_answers(dev, host, world[1])
    assert dev.search_numpy(world[1], filter=NOTHING, limit=10)[1][0].size == 0


def test_pruned_cells_over_pq_codes_gather_the_mask_through_the_table(world, tmp_path):
    from annlite_amd.core.index.ivf_pq_gpu import IvfPQGpuIndex

    x, q, tags = world
    dev, host = _pair(world, tmp_path, train=True, n_subvectors=8, n_cells=8, n_probe=3, ivf_prune=True)
    assert type(dev.vec_index(0)) is IvfPQGpuIndex and dev.vec_index(0).n_probe == 3
    _same_answers(dev, host, q)
    assert dev.vec_index(0).last_pruned_path is not None  # (the pruned search ran: its bitmap came from _table_bits)
    gone = [str(v) for v in _admitted(tags, FILTERS[0])[:30]]
    for ann in (dev, host):
        ann.delete(gone)
    _same_answers(dev, host, q)


def test_float_graph_answers_the_filter_on_the_graph(world, tmp_path):
    from annlite_amd import HnswFlatGpuIndex

    x, q, tags = world
    dev, host = _pair(world, tmp_path, graph=True, build='gpu', ef_search=96, filter_search='graph')
    assert type(dev.vec_index(0)) is HnswFlatGpuIndex
    for ann in (dev, host):
        ann.vec_index(0).FILTER_WALK_MIN_FRACTION = 0.05
    wide = [f for f in FILTERS if len(_admitted(tags, f)) >= 0.1 * N]
    assert len(wide) >= 3
    _same_answers(dev, host, q, filters=wide)
    assert dev.vec_index(0).last_filter_path == 'graph' and host.vec_index(0).last_filter_path == 'graph'
    _same_answers(dev, host, q, filters=[FEW])  # (below the floor: answered exactly, by both)
    assert dev.vec_index(0).last_filter_path == 'exact'
