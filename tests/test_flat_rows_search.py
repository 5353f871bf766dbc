"""``filter_route='rows'`` of the exact float search ("selected rows"): the selection compacted into a list of
offsets and only those rows scanned, against ``filter_route='mask'`` on the SAME index -- ids equal, distance bits equal -- for every
row type, metric and selection size at which the code takes another path (empty, fewer than k, exact-only at 4096, the filter from
4097 on, two filter stages); the mapped filter stages against the unmapped ones score by score; and what the indexes above
``FlatGpuIndex`` inherit."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

F = np.float32
N = 20_000
KINDS = {
    'f32': (dict(), 'f32', (1, 2, 3)),
    'bf16x3': (dict(flat_filter='bf16x3', centre='mean'), 'bf16x3', (1,)),  # (a centre is EUCLIDEAN's)
    'f16': (dict(dtype=np.float16), 'f16x2', (1, 2, 3)),
    'i8': (dict(dtype=np.int8), 'i8x3', (1, 2, 3)),
}


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _index(metric, D, x, **kw):
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.enums import Metric

    kw.setdefault('initial_size', max(len(x), 1))
    idx = FlatGpuIndex(D, metric=Metric(metric), **kw)
    idx.add_with_ids(x, np.arange(len(x)))
    return idx


def _same(got, want, what):
    (gd, gi), (wd, wi) = got, want
    assert gi.dtype == np.int64 and gd.dtype == np.float32
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:5], gi[gi != wi][:5], wi[gi != wi][:5])
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (what, 'distance bits')


def _mask(ops, offsets, n_rows):
    """the selection as a ``RowMask``: what a filter evaluated on the device hands the index"""
    import torch
    from annlite_amd.columns import RowMask

    bits = np.zeros((n_rows + 31) // 32 * 32, dtype=bool)
    bits[offsets] = True
    words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder='little').view(np.uint32).reshape(-1).view(np.int32)
    return RowMask(ops.to_dev(words), torch.tensor([len(offsets)]), n_rows)


def _data(D, kind):
    rs = np.random.RandomState(100 * D + len(kind))
    x = rs.randn(N, D).astype(F)
    if kind == 'i8':
        x *= 20  # (codes of a few dozen steps at the default scale of 1; COSINE normalises and stores at 2^-7)
    if kind == 'bf16x3':
        x += 50  # (a common offset: what the centre is for)
    x[100] = np.rint(x[100]).clip(-127, 127) if kind == 'i8' else np.rint(x[100] * 8) / 8  # (stored as it is by every row type: a self-match is 0.0)
    x[100:140] = x[100]  # a block of identical rows: ties ordered by id
    q = rs.randn(129, D).astype(F) * (20 if kind == 'i8' else 1) + (50 if kind == 'bf16x3' else 0)
    q[0] = x[100]  # a query equal to stored rows
    q[3, D // 2] = np.nan
    q[4, 0] = np.inf
    return rs, x, q


def _selections(rs):
    perm = rs.permutation(N)
    block = np.union1d(np.arange(100, 140), perm[:6000])  # holds the 40 identical rows
    return {
        'none': np.zeros(0, np.int64),
        'one': perm[:1],
        'nine': np.sort(perm[:9]),                 # fewer than k = 10 and 64
        'exact-only': np.sort(perm[:4096]),        # the largest list answered by exact sums
        'one-past': np.sort(perm[:4097]),          # the filter engages: 32 full row tiles and ONE row in the last
        'a-tile-more': np.sort(perm[:4225]),
        'a-third': np.flatnonzero(rs.rand(N) < 1 / 3),
        'the-end': np.arange(N - 5000, N),         # the masked search's strided sample sees almost none of it
        'ties': block,
    }


@pytest.mark.parametrize('D', [5, 33, 128])  # 5, 33: the staging of single values and a K step that is partly padding
@pytest.mark.parametrize('kind', list(KINDS))
def test_rows_route_gives_the_mask_route_its_bits(ops, kind, D):
    kw, tag, metrics = KINDS[kind]
    rs, x, q = _data(D, kind)
    sels = _selections(rs)
    for metric in metrics:
        idx = _index(metric, D, x, **kw)
        assert idx.filter_route == 'mask' and idx.last_filter_route is None
        for name, sel in sels.items():
            n_sel = len(sel)
            for B in (1, 129):
                for k in (1, 10, 64):
                    want = idx.search_batch(q[:B], limit=k, indices=sel)
                    assert idx.last_filter_route == 'mask' and idx.last_flat_filter == tag
                    got = idx.search_batch(q[:B], limit=k, indices=sel, filter_route='rows')
                    _same(got, want, (kind, metric, name, B, k))
                    assert idx.last_filter_route == 'rows'
                    assert idx.last_flat_filter == (tag if n_sel > 4096 else None), (name, idx.last_flat_filter)
                    if n_sel <= 4096:
                        assert idx.last_overflowed == 0  # (exact sums over the list: no list to overflow)
                    if n_sel == 0:
                        assert np.isinf(got[0]).all() and (got[1] == -1).all()
                    if n_sel < k:
                        assert (got[1][:, n_sel:] == -1).all() and np.isinf(got[0][:, n_sel:]).all()
            # the same selection as a device mask
            m = _mask(ops, sel, N)
            _same(idx.search_batch(q, limit=10, indices=m, filter_route='rows'), idx.search_batch(q, limit=10, indices=m), (kind, metric, name, 'mask'))
            assert idx.last_filter_route == 'mask'
        if metric == 1:  # the self-match among the ties: 0.0, and the block in id order
            d, i = idx.search_batch(q[:1], limit=64, indices=sels['ties'], filter_route='rows')
            assert d[0, 0] == 0.0 and list(i[0, :40]) == list(range(100, 140))
        # limit > 64 keeps the masked search
        _same(idx.search_batch(q[:5], limit=100, indices=sels['a-third'], filter_route='rows'),
              idx.search_batch(q[:5], limit=100, indices=sels['a-third']), (kind, metric, 'limit 100'))
        assert idx.last_filter_route == 'mask'
        # nothing to compact: no indices, no deleted rows
        idx.search_batch(q[:5], limit=10, filter_route='rows')
        assert idx.last_filter_route == 'mask' and idx.last_flat_filter == tag
        # a selection by deletes alone, and deletes under a selection
        gone = np.flatnonzero(rs.rand(N) < 0.7)
        idx.delete(gone)
        for B, k in ((129, 10), (1, 64)):
            want = idx.search_batch(q[:B], limit=k)
            assert idx.last_filter_route == 'mask'
            _same(idx.search_batch(q[:B], limit=k, filter_route='rows'), want, (kind, metric, 'deletes', B, k))
            assert idx.last_filter_route == 'rows' and idx.last_flat_filter == tag  # (about 6000 rows are left)
            assert np.isin(want[1], gone, invert=True).all()
        _same(idx.search_batch(q, limit=10, indices=sels['a-third'], filter_route='rows'), idx.search_batch(q, limit=10, indices=sels['a-third']),
              (kind, metric, 'deletes under a selection'))
        assert idx.last_filter_route == 'mask'


def test_the_constructor_keyword_and_auto(ops):
    rs, x, q = _data(33, 'f32')
    idx = _index(1, 33, x, filter_route='rows')
    sel = np.sort(rs.permutation(N)[:5000])
    got = idx.search_batch(q, limit=10, indices=sel)
    assert idx.last_filter_route == 'rows' and idx.last_flat_filter == 'f32'
    _same(got, idx.search_batch(q, limit=10, indices=sel, filter_route='mask'), 'constructor')
    assert idx.last_filter_route == 'mask'
    # 'auto': by the selection's share of the rows
    few = sel[: int(idx.ROWS_MAX_FRACTION * N) // 2]
    many = np.arange(int(idx.ROWS_MAX_FRACTION * N) + 1) if idx.ROWS_MAX_FRACTION < 1 else None
    _same(idx.search_batch(q, limit=10, indices=few, filter_route='auto'), idx.search_batch(q, limit=10, indices=few, filter_route='mask'), 'auto few')
    idx.search_batch(q, limit=10, indices=few, filter_route='auto')
    assert idx.last_filter_route == 'rows'
    if many is not None:
        idx.search_batch(q, limit=10, indices=many, filter_route='auto')
        assert idx.last_filter_route == 'mask'
    with pytest.raises(ValueError, match='filter_route'):
        idx.search_batch(q, limit=10, indices=sel, filter_route='bogus')
    # an empty index and an empty batch scan nothing
    idx.search_batch(q[:0], limit=10, indices=sel)
    assert idx.last_filter_route is None


def test_growth_reallocates_the_list(ops):
    rs = np.random.RandomState(7)
    x = rs.randn(9000, 16).astype(F)
    q = rs.randn(8, 16).astype(F)
    idx = _index(1, 16, x[:3000], filter_route='rows', initial_size=3000, expand_step_size=3000)
    sel = np.arange(0, 3000, 2)
    idx.search_batch(q, limit=10, indices=sel)
    assert idx._sel_rows.numel() >= 3000
    idx.add_with_ids(x[3000:], np.arange(3000, 9000))
    sel = np.arange(1, 9000, 2)
    _same(idx.search_batch(q, limit=10, indices=sel), idx.search_batch(q, limit=10, indices=sel, filter_route='mask'), 'grown')
    assert idx._sel_rows.numel() >= 9000


# ---- two filter stages ----------------------------------------------------------------------------------------------------------------
def test_several_filter_stages_and_no_overflow(ops):
    """N = 300 000 with about 150 000 rows selected: more than 32 x 4096, so the mapped filter runs in two stages.  i.i.d. normal data:
    lists of a few hundred entries against a capacity of 4096."""
    rs = np.random.RandomState(5)
    n, D, B = 300_000, 16, 64
    x = rs.randn(n, D).astype(F)
    q = rs.randn(B, D).astype(F)
    idx = _index(1, D, x)
    sel = np.flatnonzero(rs.rand(n) < 0.5)
    assert len(sel) > 32 * 4096
    m = _mask(ops, sel, n)
    sub = np.arange(0, B, 4)  # 16 of the queries
    for k in (10, 64):
        got = idx.search_batch(q, limit=k, indices=m, filter_route='rows')
        assert idx.last_filter_route == 'rows' and idx.last_flat_filter == 'f32' and idx.last_overflowed == 0
        want = idx.search_batch(q[sub], limit=k, indices=m)
        _same((got[0][sub], got[1][sub]), want, k)
        assert np.isin(got[1], sel).all()


# ---- the mapped stages, score by score ------------------------------------------------------------------------------------------------
def _stage_world(ops, kind, metric, D):
    n, B = 300, 130  # (3 row tiles of the table, 2 of the list, 2 query tiles, all with a ragged edge)
    rs = np.random.RandomState(D + 10 * metric)
    x = rs.randn(n, D).astype(F)
    q = rs.randn(B, D).astype(F)
    rows = np.sort(rs.permutation(n)[:130]).astype(np.int32)
    qd = ops.to_dev(q)
    w = dict(n=n, B=B, rows=rows, rows_dev=ops.to_dev(rows), q=qd, centre=None, scale=1.0)
    if kind == 'f16x2':
        w['x'] = ops.to_dev(x.astype(np.float16))
        w['norms'] = ops.flat_row_norms_f16(w['x'])
        w['unmapped'] = lambda bounds: ops.flat_filter_f16(metric, qd, w['x'], w['norms'], bounds, scores=True)
        w['exact'] = lambda cand: ops.exact_gather_dist_f16(metric, qd, w['x'], cand)
    elif kind == 'i8x3':
        w['scale'] = 2.0 ** -5
        w['x'] = ops.to_dev(np.clip(np.rint(x * 32), -127, 127).astype(np.int8))
        w['norms'] = ops.flat_row_norms_i8(w['x'], w['scale'])
        w['unmapped'] = lambda bounds: ops.flat_filter_i8(metric, qd, w['x'], w['norms'], bounds, w['scale'], scores=True)
        w['exact'] = lambda cand: ops.exact_gather_dist_i8(metric, qd, w['x'], cand, w['scale'])
    else:
        w['x'] = ops.to_dev(x + (30 if metric == 1 else 0))
        if metric == 1:
            w['q'] = qd = ops.to_dev(q + 30)
            w['centre'] = w['x'].mean(dim=0).contiguous()
            w['norms'] = ops.flat_centred_norms(w['x'], w['centre'])
        else:
            w['norms'] = ops.flat_row_norms(w['x'])
        w['unmapped'] = lambda bounds: ops.flat_filter_split(metric, qd, w['x'], w['norms'], bounds, centre=w['centre'], scores=True)
        w['exact'] = lambda cand: ops.exact_gather_dist(metric, qd, w['x'], cand)
    return w


@pytest.mark.parametrize('D', [5, 40, 128])
@pytest.mark.parametrize('metric', [1, 2])
@pytest.mark.parametrize('kind', ['f16x2', 'i8x3', 'bf16x3'])
def test_mapped_stage_scores_are_the_unmapped_ones(ops, kind, metric, D):
    import torch

    w = _stage_world(ops, kind, metric, D)
    B, rows = w['B'], w['rows']
    inf = torch.full((B,), float('inf'), device=w['q'].device)
    mapped = lambda bounds: ops.flat_filter_rows(kind, metric, w['q'], w['x'], w['norms'], bounds, w['rows_dev'], centre=w['centre'],
                                                 scale=w['scale'], scores=True)
    # the same contraction per (query, row) pair: the score by list position is the score of that table row, bit for bit
    sc_table = w['unmapped'](inf)[-1].cpu().numpy()
    cand, count, sc = mapped(inf)
    assert sc.shape == (B, len(rows))
    assert np.array_equal(sc.cpu().numpy().view(np.uint32), sc_table[:, rows].view(np.uint32))
    # an infinite bound lists the list, no row twice, none from outside
    cand, count = cand.cpu().numpy(), count.cpu().numpy()
    assert (count == len(rows)).all()
    for b in (0, 1, 64, 127, 128, 129):
        assert np.array_equal(np.sort(cand[b, :len(rows)]), rows)
    # a finite bound: every list row whose exact distance is within it is a candidate; nothing outside the list ever is
    exact = w['exact'](torch.from_numpy(rows.astype(np.int64))[None, :].expand(B, -1).contiguous().to(w['q'].device)).cpu().numpy()
    bound = np.sort(exact, axis=1)[:, 40].copy()  # (the 41st smallest of 130)
    cand, count = (t.cpu().numpy() for t in mapped(ops.to_dev(bound))[:2])
    for b in range(B):
        listed = cand[b, :count[b]]
        assert np.isin(listed, rows).all() and len(np.unique(listed)) == len(listed), b
        assert np.isin(rows[exact[b] <= bound[b]], listed).all(), b
        assert count[b] < len(rows), b  # (the filter filters: not everything passes a bound at the 41st)
    # a stride over the list
    sc2 = ops.flat_filter_rows(kind, metric, w['q'], w['x'], w['norms'], inf, w['rows_dev'], centre=w['centre'], scale=w['scale'], stride=3,
                               scores=True)[2].cpu().numpy()
    assert np.array_equal(sc2.view(np.uint32), sc_table[:, rows[::3]].view(np.uint32))


def test_the_f32_stage_lists_the_rows_within_the_bound(ops):
    import torch

    metric, D = 1, 33
    rs = np.random.RandomState(11)
    x, q = rs.randn(300, D).astype(F), rs.randn(130, D).astype(F)
    rows = np.sort(rs.permutation(300)[:130]).astype(np.int32)
    xd, qd = ops.to_dev(x), ops.to_dev(q)
    norms = ops.flat_row_norms(xd)
    exact = ops.exact_gather_dist(metric, qd, xd, torch.from_numpy(rows.astype(np.int64))[None, :].expand(130, -1).contiguous().to(qd.device))
    exact = exact.cpu().numpy()
    bound = np.sort(exact, axis=1)[:, 40].copy()
    cand, count = (t.cpu().numpy() for t in ops.flat_filter_rows('f32', metric, qd, xd, norms, ops.to_dev(bound), ops.to_dev(rows)))
    for b in range(130):
        listed = cand[b, :count[b]]
        assert np.isin(listed, rows).all() and np.isin(rows[exact[b] <= bound[b]], listed).all() and count[b] < 130
    with pytest.raises(Exception):
        ops.flat_filter_rows('f32', metric, qd, xd, norms, ops.to_dev(bound), ops.to_dev(rows), scores=True)  # (the f32 kernel has no scores)


# ---- what the indexes above inherit -----------------------------------------------------------------------------------------------------
def test_the_float_graph_inherits_the_route_in_its_exact_fallback(ops):
    from annlite_amd.core.index.hnsw_flat_gpu import HnswFlatGpuIndex
    from annlite_amd.enums import Metric

    rs = np.random.RandomState(21)
    n, D = 6000, 16
    x, q = rs.randn(n, D).astype(F), rs.randn(32, D).astype(F)
    hn = HnswFlatGpuIndex(D, metric=Metric.EUCLIDEAN, initial_size=n, filter_search='graph', filter_route='rows')
    hn.add_with_ids(x, np.arange(n))
    few = np.sort(rs.permutation(n)[: n // 50])  # 2 %: below FILTER_WALK_MIN_FRACTION, the exact fallback
    got = hn.search_batch(q, limit=10, indices=few)
    assert hn.last_filter_path == 'exact' and hn.last_filter_route == 'rows'
    want = hn.search_batch(q, limit=10, indices=few, filter_route='mask')
    assert hn.last_filter_route == 'mask'
    _same(got, want, 'graph')
    _same(hn.search_exhaustive(q, limit=10, indices=few), want, 'search_exhaustive')
    assert hn.last_filter_route == 'rows'
    hn.search_batch(q, limit=10)  # (a walk scans no table)
    assert hn.last_filter_route is None


def test_the_cells_inherit_the_route_in_the_every_cell_search(ops):
    from annlite_amd.core.codec.vq import VQCodec
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex
    from annlite_amd.enums import Metric

    rs = np.random.RandomState(22)
    n, D, C = 12_000, 16, 4
    x, q = rs.randn(n, D).astype(F), rs.randn(32, D).astype(F)
    vq = VQCodec(C, metric=Metric.EUCLIDEAN)
    vq._codebook = rs.randn(C, D).astype(F)
    vq._is_trained = True
    idx = IvfFlatGpuIndex(D, vq_codec=vq, n_probe=None, metric=Metric.EUCLIDEAN, initial_size=n, filter_route='rows')
    idx.add_with_ids(x, np.arange(n))
    sel = np.flatnonzero(rs.rand(n) < 0.45)  # more than 4096 rows: the mapped filter runs
    got = idx.search_batch(q, limit=10, indices=sel)
    assert idx.last_filter_route == 'rows' and idx.last_flat_filter == 'f32'
    _same(got, idx.search_batch(q, limit=10, indices=sel, filter_route='mask'), 'every cell')
    idx.search_batch(q, limit=10, indices=sel, n_probe=2)  # the pruned search: cell tiles under the bitmap
    assert idx.last_filter_route == 'mask'


def test_the_facade_hands_the_keyword_down(ops, tmp_path):
    from annlite_amd import AnnLite
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.index import Document, DocumentArray

    rs = np.random.RandomState(23)
    n, D = 6000, 16
    x, q = rs.randn(n, D).astype(F), rs.randn(8, D).astype(F)
    docs = lambda: DocumentArray([Document(id=str(r), embedding=x[r], tags={'a': int(r % 10)}) for r in range(n)])
    new = AnnLite(D, metric='euclidean', data_path=tmp_path / 'rows', columns=[('a', int)], filter_route='rows')
    old = AnnLite(D, metric='euclidean', data_path=tmp_path / 'mask', columns=[('a', int)])
    for ann in (new, old):
        ann.index(docs())
        assert type(ann.vec_index(0)) is FlatGpuIndex
    flt = {'a': {'$lt': 3}}
    (gd, gi), (wd, wi) = new.search_numpy(q, filter=flt, limit=10), old.search_numpy(q, filter=flt, limit=10)
    assert new.vec_index(0).last_filter_route == 'rows' and old.vec_index(0).last_filter_route == 'mask'
    assert new.last_filter_eval == 'gpu'
    for b in range(len(q)):
        assert np.array_equal(gi[b], wi[b]) and np.array_equal(np.asarray(gd[b]).view(np.uint32), np.asarray(wd[b]).view(np.uint32))
        assert (np.asarray(gi[b]) % 10 < 3).all()
