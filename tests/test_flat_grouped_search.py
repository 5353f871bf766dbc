"""A filter per query in one batch ("a filter per query"): ``search_batch_grouped`` against the single-filter
``search_batch(indices=...)`` per group on the SAME index, the grouped filter stage against the ungrouped stages under each group's mask,
the routes that loop or split, and the facade's ``filter=[...]``.  Ids are compared by ``array_equal`` and distances by their bits: there
is no tolerance and no query is left out."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

F = np.float32
N, B, G = 9000, 130, 6  # one filter stage (above FILTER_MIN_ROWS); two query tiles, the second nearly empty
TIES = np.arange(100, 140)  # a block of identical rows
KINDS = {
    'f32': (lambda metric: dict(), 'f32'),
    'bf16x3': (lambda metric: dict(flat_filter='bf16x3', centre='mean'), 'bf16x3'),  # (the centre is EUCLIDEAN's; 2 / 3 run it uncentred)
    'f16': (lambda metric: dict(dtype=np.float16), 'f16x2'),
    'i8': (lambda metric: dict(dtype=np.int8, int8_scale=2.0 ** -6 if metric == 3 else 0.5), 'i8x3'),
}


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _index(metric, D, x, cls=None, **kw):
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.enums import Metric

    kw.setdefault('initial_size', max(len(x), 1))
    idx = (cls or FlatGpuIndex)(D, metric=Metric(metric), **kw)
    if len(x):
        idx.add_with_ids(x, np.arange(len(x)))
    return idx


def _same(got, want, what):
    (gd, gi), (wd, wi) = got, want
    assert gi.dtype == np.int64 and gd.dtype == np.float32 and gi.shape == wi.shape
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:5], gi[gi != wi][:5], wi[gi != wi][:5])
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (what, 'distance bits')


def _words(offsets, n_rows):
    bits = np.zeros((n_rows + 31) // 32 * 32, dtype=bool)
    bits[offsets] = True
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder='little').view(np.uint32).reshape(-1).view(np.int32)


def _mask(ops, offsets, n_rows):
    """the selection as a ``RowMask``: what a filter evaluated on the device hands the index"""
    import torch
    from annlite_amd.columns import RowMask

    return RowMask(ops.to_dev(_words(offsets, n_rows)), torch.tensor([len(offsets)]), n_rows)


def _world(D, kind, n=N, nq=B):
    rs = np.random.RandomState(1000 * D + len(kind))
    scale = 10 if kind == 'i8' else 1
    x = rs.randn(n, D).astype(F) * scale + (50 if kind == 'bf16x3' else 0)  # (a common offset: what the centre is for)
    x[TIES[0]] = np.rint(x[TIES[0]])  # (stored as it is by every row type: a self-match is 0.0)
    x[TIES] = x[TIES[0]]
    q = rs.randn(nq, D).astype(F) * scale + (50 if kind == 'bf16x3' else 0)
    q[1] = x[TIES[0]]  # group 1 (the half): a query equal to the block
    perm = rs.permutation(n)
    gone = np.setdiff1d(perm[:50], np.concatenate([TIES, [31, 32, 63, 64, n - 1]]))  # about 50 deleted rows
    return rs, x, q, gone


def _selections(ops, rs, n, gone, k):
    """the six of the issue; as search_batch takes them -- None, a RowMask, offsets"""
    half = np.union1d(np.flatnonzero(rs.rand(n) < 0.5), TIES)
    tenth = np.flatnonzero(rs.rand(n) < 0.1)
    alive = np.setdiff1d(np.arange(n), gone)
    return [None, _mask(ops, half, n), tenth, np.sort(rs.permutation(alive)[:k - 1]), np.zeros(0, np.int64),
            np.array([31, 32, 63, 64, n - 1, gone[0]])], half


def _per_group(idx, q, k, sels, group_of, to_dev=None, **kw):
    """the yardstick: one single-filter ``search_batch`` per group, scattered back (``_per_group.overflowed``: their overflowed queries).
    ``to_dev``: hand the queries over as device tensors (COSINE normalises those on the device, host arrays on the host)"""
    d = np.full((len(q), k), np.inf, F)
    i = np.full((len(q), k), -1, np.int64)
    _per_group.overflowed = 0
    for g in np.unique(group_of):
        at = np.flatnonzero(group_of == g)
        if to_dev is None:
            d[at], i[at] = idx.search_batch(q[at], limit=k, indices=sels[g], **kw)
        else:
            d[at], i[at] = (t.cpu().numpy() for t in idx.search_batch(to_dev(q[at]), limit=k, indices=sels[g], **kw))
        _per_group.overflowed += getattr(idx, 'last_overflowed', 0)
    return d, i


# ---- 1. end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [5, 96])  # scalar staging and the vector path
@pytest.mark.parametrize('metric', [1, 2, 3])
@pytest.mark.parametrize('kind', list(KINDS))
def test_grouped_search_is_the_search_per_group(ops, kind, metric, D):
    kw, tag = KINDS[kind]
    rs, x, q, gone = _world(D, kind)
    idx = _index(metric, D, x, **kw(metric))
    idx.delete(gone)
    group_of = np.arange(B) % G  # every 32 x 32 C tile mixes all groups
    for k in (1, 10, 64):
        sels, half = _selections(ops, rs, N, gone, k)
        want = _per_group(idx, q, k, sels, group_of)
        got = idx.search_batch_grouped(q, limit=k, selections=sels, group_of=group_of)
        assert idx.last_filter_batch == 'grouped' and idx.last_flat_filter == tag and idx.last_filter_route == 'mask'
        assert idx.last_overflowed == _per_group.overflowed  # (the same bounds and lists per query: the same queries overflow)
        _same(got, want, (kind, metric, D, k))
        d, i = got
        assert not np.isin(i, gone).any()  # the deleted row of the sixth selection does not come back
        assert (i[group_of == 4] == -1).all() and np.isinf(d[group_of == 4]).all()
        assert ((i[group_of == 3] >= 0).sum(axis=1) == min(k, k - 1)).all()
        assert ((i[group_of == 5] >= 0).sum(axis=1) == min(k, 5)).all() and np.isin(i[group_of == 5], [31, 32, 63, 64, N - 1, -1]).all()
        assert np.isin(i[group_of == 1], np.append(half, -1)).all()
        if metric == 1 and k == 64:  # duplicated rows inside a mask come out in id order
            assert d[1, 0] == 0.0 and list(i[1, :len(TIES)]) == list(TIES)
    # device tensors in, device tensors out; a list for group_of
    import torch

    td, ti = idx.search_batch_grouped(ops.to_dev(q), limit=10, selections=sels, group_of=list(group_of))
    assert isinstance(td, torch.Tensor) and td.is_cuda
    _same((td.cpu().numpy(), ti.cpu().numpy()), _per_group(idx, q, 10, sels, group_of, to_dev=ops.to_dev), 'tensors')


def test_several_filter_stages(ops):
    """N = 140 000: two filter stages.  Masks of 50 / 10 / 1 %; the last keeps about 40 of the 4096 sampled rows -- fewer than k = 64: its
    queries get the bound +inf, and their lists take the mask's 1400 rows."""
    rs = np.random.RandomState(5)
    n, D, nq = 140_000, 16, 64
    x, q = rs.randn(n, D).astype(F), rs.randn(nq, D).astype(F)
    idx = _index(1, D, x)
    sels = [_mask(ops, np.flatnonzero(rs.rand(n) < p), n) for p in (0.5, 0.1, 0.01)]
    group_of = np.arange(nq) % 3
    for k in (10, 64):
        got = idx.search_batch_grouped(q, limit=k, selections=sels, group_of=group_of)
        assert idx.last_filter_batch == 'grouped' and idx.last_flat_filter == 'f32'
        over = idx.last_overflowed
        _same(got, _per_group(idx, q, k, sels, group_of), k)
        assert over == _per_group.overflowed == 0  # (i.i.d. normal data, and a mask of 1400 rows fits a list whatever the bound)


# ---- 2. the stage ----------------------------------------------------------------------------------------------------------------------
def _stage_world(ops, kind, metric, D):
    rs, x, q, gone = _world(D, kind)
    qd = ops.to_dev(q)
    w = dict(q=qd, centre=None, scale=1.0, rs=rs, gone=gone)
    if kind == 'f16':
        w['x'] = ops.to_dev(x.astype(np.float16))
        w['norms'] = ops.flat_row_norms_f16(w['x'])
        w['single'] = lambda bounds, valid: ops.flat_filter_f16(metric, qd, w['x'], w['norms'], bounds, valid_bits=valid)
        w['exact'] = lambda cand: ops.exact_gather_dist_f16(metric, qd, w['x'], cand)
    elif kind == 'i8':
        w['scale'] = 0.5
        w['x'] = ops.to_dev(np.clip(np.rint(x * 2), -127, 127).astype(np.int8))
        w['norms'] = ops.flat_row_norms_i8(w['x'], w['scale'])
        w['single'] = lambda bounds, valid: ops.flat_filter_i8(metric, qd, w['x'], w['norms'], bounds, w['scale'], valid_bits=valid)
        w['exact'] = lambda cand: ops.exact_gather_dist_i8(metric, qd, w['x'], cand, w['scale'])
    else:
        w['x'] = ops.to_dev(x)
        w['exact'] = lambda cand: ops.exact_gather_dist(metric, qd, w['x'], cand)
        if kind == 'bf16x3':
            if metric == 1:
                w['centre'] = w['x'].mean(dim=0).contiguous()
                w['norms'] = ops.flat_centred_norms(w['x'], w['centre'])
            else:
                w['norms'] = ops.flat_row_norms(w['x'])
            w['single'] = lambda bounds, valid: ops.flat_filter_split(metric, qd, w['x'], w['norms'], bounds, centre=w['centre'], valid_bits=valid)
        else:
            w['norms'] = ops.flat_row_norms(w['x'])
            w['single'] = lambda bounds, valid: ops.flat_filter(metric, qd, w['x'], w['norms'], bounds, valid_bits=valid)
    return w


@pytest.mark.parametrize('D', [5, 96])
@pytest.mark.parametrize('metric', [1, 2])
@pytest.mark.parametrize('kind', list(KINDS))
def test_grouped_stage_lists_what_the_ungrouped_stage_lists_under_each_mask(ops, kind, metric, D):
    import torch

    w = _stage_world(ops, kind, metric, D)
    k = 10
    sels, _ = _selections(ops, w['rs'], N, w['gone'], k)
    live = np.setdiff1d(np.arange(N), w['gone'])
    rows_of = [live, np.intersect1d(sels[1].offsets(), live), np.intersect1d(sels[2], live), sels[3], sels[4], np.intersect1d(sels[5], live)]
    assert len(rows_of[5]) == 5 and len(rows_of[3]) == k - 1
    # (the host ANDs the live bitmap in)
    masks = ops.to_dev(np.stack([_words(r, N) for r in rows_of]))
    valid = ops.to_dev(_words(live, N))
    group_of = (np.arange(B) % G).astype(np.int32)
    group_of[[12, 13]] = -1, G  # ids outside [0, G): they select nothing
    # the bounds of a first sample: the k-th smallest exact distance among every second row of the query's mask (+inf: fewer than k)
    sample = np.arange(0, N, 2)
    dist = w['exact'](torch.from_numpy(sample)[None, :].expand(B, -1).contiguous().to(w['q'].device)).cpu().numpy()
    bounds = np.full(B, np.inf, F)
    for b in range(B):
        if 0 <= group_of[b] < G:
            mine = np.sort(dist[b, np.isin(sample, rows_of[group_of[b]])])
            if len(mine) >= k:
                bounds[b] = mine[k - 1]
    bounds_dev = ops.to_dev(bounds)
    tag = KINDS[kind][1]
    cand, count = (t.cpu().numpy() for t in ops.flat_filter_grouped(tag, metric, w['q'], w['x'], w['norms'], bounds_dev, masks, ops.to_dev(group_of),
                                                                    valid_bits=valid, centre=w['centre'], scale=w['scale'])[:2])
    cap = ops.flat_list_capacity()
    single = [tuple(t.cpu().numpy() for t in w['single'](bounds_dev, masks[g])[:2]) for g in range(G)]
    n_finite = 0
    for b in range(B):
        g = group_of[b]
        if not 0 <= g < G:
            assert count[b] == 0, (b, g)
            continue
        want_cand, want_count = single[g]
        assert count[b] == want_count[b], (b, g, count[b], want_count[b])
        if count[b] > cap:  # (an overflowed list: the tail was not stored by either stage)
            continue
        listed, want = cand[b, :count[b]], want_cand[b, :want_count[b]]
        assert len(np.unique(listed)) == len(listed), (b, 'a row twice')
        assert np.isin(listed, rows_of[g]).all(), (b, 'a row outside the mask')
        assert np.array_equal(np.sort(listed), np.sort(want)), (b, g)
        if np.isfinite(bounds[b]):
            n_finite += 1
            assert k <= count[b] < len(rows_of[g]), (b, g, count[b])  # (the filter filters, and the sample's k rows pass)
        else:
            assert count[b] == len(rows_of[g])  # (an infinite bound lists the mask)
    assert n_finite >= B // 3
    if tag == 'f32':
        with pytest.raises(Exception):
            ops.flat_filter_grouped(tag, metric, w['q'], w['x'], w['norms'], bounds_dev, masks, ops.to_dev(group_of), valid_bits=valid, scores=True)
    else:  # the scores are the ungrouped stage's: the contraction does not know about groups
        sc = ops.flat_filter_grouped(tag, metric, w['q'], w['x'], w['norms'], bounds_dev, masks, ops.to_dev(group_of), valid_bits=valid,
                                     centre=w['centre'], scale=w['scale'], scores=True)[2].cpu().numpy()
        assert sc.shape == (B, N) and not np.isnan(sc[:, live]).any()


# ---- 3. routes -------------------------------------------------------------------------------------------------------------------------
def test_a_large_limit_loops_and_many_groups_split(ops):
    rs, x, q, gone = _world(16, 'f32')
    idx = _index(1, 16, x)
    idx.delete(gone)
    group_of = np.arange(B) % G
    sels, _ = _selections(ops, rs, N, gone, 10)
    got = idx.search_batch_grouped(q, limit=100, selections=sels, group_of=group_of)
    assert idx.last_filter_batch == 'looped'
    _same(got, _per_group(idx, q, 100, sels, group_of), 'limit 100')
    # 70 single-row masks (and two that no query uses): more than MAX_FILTER_GROUPS bitmaps, two launches
    assert idx.MAX_FILTER_GROUPS == 64
    alive = np.setdiff1d(np.arange(N), gone)
    many = [alive[7 * g:7 * g + 1] for g in range(72)]
    group_of = np.arange(140) % 70
    q2 = np.concatenate([q, q[:10]])
    got = idx.search_batch_grouped(q2, limit=10, selections=many, group_of=group_of)
    assert idx.last_filter_batch == 'grouped'
    over = idx.last_overflowed  # (summed over the launches)
    _same(got, _per_group(idx, q2, 10, many, group_of), '70 groups')
    assert over == _per_group.overflowed == 0
    assert np.array_equal(got[1][:, 0], np.array([many[g][0] for g in group_of])) and (got[1][:, 1:] == -1).all()
    # group ids are checked on the host
    with pytest.raises(ValueError, match='group_of'):
        idx.search_batch_grouped(q, limit=10, selections=sels, group_of=np.full(B, G))
    with pytest.raises(ValueError, match='group_of'):
        idx.search_batch_grouped(q, limit=10, selections=sels, group_of=group_of[:5])
    # an empty batch
    d, i = idx.search_batch_grouped(q[:0], limit=10, selections=sels, group_of=[])
    assert d.shape == (0, 10) and i.shape == (0, 10)


def test_the_pruned_and_the_graph_index_loop(ops):
    from annlite_amd.core.codec.vq import VQCodec
    from annlite_amd.core.index.hnsw_flat_gpu import HnswFlatGpuIndex
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex
    from annlite_amd.enums import Metric

    rs = np.random.RandomState(22)
    n, D, C = 12_000, 16, 4
    x, q = rs.randn(n, D).astype(F), rs.randn(32, D).astype(F)
    sels = [None, _mask(ops, np.flatnonzero(rs.rand(n) < 0.45), n), np.sort(rs.permutation(n)[:n // 50]), np.zeros(0, np.int64)]
    group_of = np.arange(32) % 4
    vq = VQCodec(C, metric=Metric.EUCLIDEAN)
    vq._codebook = rs.randn(C, D).astype(F)
    vq._is_trained = True
    ivf = IvfFlatGpuIndex(D, vq_codec=vq, n_probe=2, metric=Metric.EUCLIDEAN, initial_size=n)
    ivf.add_with_ids(x, np.arange(n))
    got = ivf.search_batch_grouped(q, limit=10, selections=sels, group_of=group_of)
    assert ivf.last_filter_batch == 'looped'
    _same(got, _per_group(ivf, q, 10, sels, group_of), 'cells, n_probe = 2 of 4')
    exhaustive = _index(1, D, x).search_batch_grouped(q, limit=10, selections=sels, group_of=group_of)
    assert not np.array_equal(got[1], exhaustive[1])  # (the pruned search stayed pruned)
    hn = HnswFlatGpuIndex(D, metric=Metric.EUCLIDEAN, initial_size=n)
    hn.add_with_ids(x[:6000], np.arange(6000))
    hsels = [None, _mask(ops, np.flatnonzero(rs.rand(6000) < 0.45), 6000), np.sort(rs.permutation(6000)[:120]), np.zeros(0, np.int64)]
    got = hn.search_batch_grouped(q, limit=10, selections=hsels, group_of=group_of)
    assert hn.last_filter_batch == 'looped'
    _same(got, _per_group(hn, q, 10, hsels, group_of), 'graph')


def test_an_empty_index_answers_nothing(ops):
    rs = np.random.RandomState(1)
    q = rs.randn(7, 8).astype(F)
    idx = _index(1, 8, np.zeros((0, 8), F), initial_size=64)
    d, i = idx.search_batch_grouped(q, limit=5, selections=[None, np.array([1, 2])], group_of=[0, 1, 0, 1, 0, 1, 1])
    assert d.shape == (7, 5) and np.isinf(d).all() and (i == -1).all() and d.dtype == F and i.dtype == np.int64


# ---- 4. the facade ---------------------------------------------------------------------------------------------------------------------
def test_the_facade_takes_a_filter_per_query(ops, tmp_path):
    from annlite_amd import AnnLite
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.index import Document, DocumentArray

    rs = np.random.RandomState(23)
    n, D, nq = 6000, 32, 40
    x, q = rs.randn(n, D).astype(F), rs.randn(nq, D).astype(F)
    tags = [{'tenant': int(r % 11), 'x': (r * 7919 % n) / n, 'colour': ['red', 'blue'][r % 2]} for r in range(n)]  # ('colour' is not declared)
    ann = AnnLite(D, metric='euclidean', data_path=tmp_path, columns=[('tenant', int), ('x', float)])
    ann.index(DocumentArray([Document(id=str(r), embedding=x[r], tags=tags[r]) for r in range(n)]))
    assert type(ann.vec_index(0)) is FlatGpuIndex
    ann.delete([str(r) for r in range(0, n, 97)])
    distinct = [{'tenant': {'$eq': 3}}, {'tenant': {'$lt': 4}, 'x': {'$gt': 0.25}}, {'x': {'$lt': 2.5 / n}}, {'tenant': {'$gt': 100}},
                {'colour': 'red', 'tenant': {'$gte': 5}}, None]
    filters = [distinct[b % 6] if b % 12 else dict(distinct[0]) for b in range(nq)]  # (an equal dict that is another object)
    filters[5] = {}  # ({} is None)
    for limit in (10, 3):
        gd, gi = ann.search_numpy(q, filter=filters, limit=limit)
        assert ann.last_filter_groups == 6 and ann.last_filter_batch == 'grouped' and ann.last_filter_eval == 'host'
        assert len(gd) == len(gi) == nq
        lengths = set()
        for b in range(nq):
            wd, wi = ann.search_numpy(q[b:b + 1], filter=filters[b], limit=limit)
            assert ann.last_filter_batch is None and ann.last_filter_groups is None
            assert np.array_equal(gi[b], wi[0]) and gi[b].dtype == wi[0].dtype, b
            assert np.array_equal(np.asarray(gd[b], F).view(np.uint32), np.asarray(wd[0], F).view(np.uint32)), b
            lengths.add(len(gi[b]))
        assert 0 in lengths and limit in lengths and lengths & {1, 2}  # (no row, fewer rows than the limit, a full list)
    # without the host filter: every filter is evaluated on the device, once
    on_device = [f for f in filters if not (f and 'colour' in f)]
    ann.search_numpy(q[:len(on_device)], filter=on_device)
    assert ann.last_filter_eval == 'gpu' and ann.last_filter_groups == 5 and ann.last_filter_batch == 'grouped'
    # a list of B equal dicts is the dict passed once
    flt = distinct[1]
    (gd, gi), (wd, wi) = ann.search_numpy(q, filter=[dict(flt) for _ in range(nq)]), ann.search_numpy(q, filter=flt)
    assert ann.last_filter_batch is None
    for b in range(nq):
        assert np.array_equal(gi[b], wi[b]) and np.array_equal(np.asarray(gd[b]).view(np.uint32), np.asarray(wd[b]).view(np.uint32))
    ann.search_numpy(q, filter=[dict(flt) for _ in range(nq)])
    assert ann.last_filter_groups == 1 and ann.last_filter_batch is None
    # a wrong length
    for bad in (filters[:-1], filters + [None], []):
        with pytest.raises(ValueError, match='one filter per query'):
            ann.search_numpy(q, filter=bad)
    # search(docs, filter=[...]) attaches the same matches
    docs = DocumentArray([Document(id=f'q{b}', embedding=q[b]) for b in range(nq)])
    ann.search(docs, filter=tuple(filters), limit=10)
    assert ann.last_filter_batch == 'grouped'
    gd, gi = ann.search_numpy(q, filter=filters, limit=10)
    for b, doc in enumerate(docs):
        assert [int(m.id) for m in doc.matches] == list(gi[b]), b
        assert [np.float32(m.scores['euclidean'].value) for m in doc.matches] == [np.float32(v) for v in gd[b]], b
        if filters[b] and 'tenant' in filters[b] and '$eq' in filters[b]['tenant']:
            assert all(m.tags['tenant'] == 3 for m in doc.matches)
