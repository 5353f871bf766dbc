"""Cells over int8 rows (``IvfFlatGpuIndex(ivf_rows='i8')``; DESIGN.md section 3.7, "int8 rows over cell tiles") against numpy float64
over the decoded rows ``s * c`` of each query's probed cells (``_truth`` of test_flat_ground_truth.py) and, bit for bit, against the f32
cell index that holds the decoded rows (``_pair``).  EUCLIDEAN / INNER_PRODUCT run at ``int8_scale = 2**-3`` -- the helpers' coordinates
reach about 8.5, inside +-15.9, the noise is 2 to 3 code steps, exact ties are plenty --, COSINE at its default ``2**-7``."""
import numpy as np
import pytest

from conftest import has_gpu
from test_flat_ground_truth import _truth, ops  # noqa: F401 (the fixture)
from test_flat_i8_search import _digits
from test_ivf_flat_search import SIZES, _centroids, _index, _probed, _queries, _rows, _same, _vq

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]
F, I8 = np.float32, np.int8
SCALE = {1: 2.0 ** -3, 2: 2.0 ** -3, 3: None}


def dec(x, s):
    """the f32 rows an int8 store of scale ``s`` holds for ``x``"""
    return (F(s) * np.clip(np.rint(x / F(s)), -127, 127)).astype(F)


def _pre(metric, x):
    from annlite_amd.math import l2_normalize_host

    return l2_normalize_host(x) if metric == 3 else x


def _pair(ops, metric, D, vq, x, **kw):
    """(the int8 index over x, the f32 index over the decoded rows, sync).  COSINE stores the normalised vector quantised, which a COSINE
    f32 index would normalise again: it is given the decoded rows (same cells, same probes) and sync() hands it the int8 index's rows."""
    new = _index(metric, D, vq, x, ivf_rows='i8', int8_scale=SCALE[metric], **kw)
    s = new.int8_scale_
    ref = _index(metric, D, vq, dec(_pre(metric, x), s), **kw)

    def sync():
        n = new._n_rows
        assert ref._n_rows == n and np.array_equal(new._cell_of[:n].cpu().numpy(), ref._cell_of[:n].cpu().numpy())
        if metric == 3:
            ref._vectors[:n] = new._vectors[:n].float() * s
            ops.flat_row_norms(ref._vectors, n=n, out=ref._norms)
    sync()
    return new, ref, sync


# byte staging and a padded Dp; byte staging, a partial second K step; VEC, a second stage of one K step; VEC, two full stages
@pytest.mark.parametrize('D', [5, 40, 96, 128])
@pytest.mark.parametrize('metric', [1, 2, 3])
def test_answer_against_float64_over_the_decoded_rows(ops, metric, D):
    C, P, B = len(SIZES), 3, 130
    rs = np.random.RandomState(7 * D + metric)
    x, q = _rows(rs, SIZES, D)[0], _queries(rs, C, D, B)
    idx = _index(metric, D, _vq(C, D, metric), x, ivf_rows='i8', int8_scale=SCALE[metric], n_probe=P)
    s = idx.int8_scale_
    codes = np.clip(np.rint(_pre(metric, x) / F(s)), -127, 127).astype(I8)
    assert np.array_equal(idx._vectors[:len(x)].cpu().numpy(), codes)  # rounded once, to nearest even, byte for byte

    def judge(live, what, **kw):
        qd, cand, _ = _probed(idx, q, P)
        T, E = _truth(metric, s * codes.astype(np.float64), qd.cpu().numpy().astype(np.float64))
        cand = cand.cpu().numpy()
        for k in (1, 10, 64):
            d, i = idx.search_batch(q, limit=k, **kw)
            assert idx.last_cell_filter == 'i8x3'
            for b in range(B):
                rows = cand[b][cand[b] >= 0]
                rows = rows[live[rows]]
                kk = min(k, len(rows))
                got = i[b, :kk]
                assert (i[b, kk:] == -1).all() and np.isposinf(d[b, kk:]).all(), (what, k, b)
                assert len(set(got.tolist())) == kk and np.isin(got, rows).all(), (what, k, b, 'ids distinct, live and probed')
                # by rank: the computed distances lie within E of the truth, so their j-th smallest lies within max E of the truth's
                # (COSINE assigns the cells from normalised rows, all next to one corner: a query may probe empty cells alone)
                worst = E[b, rows].max() if len(rows) else 0.0
                assert (np.abs(T[b, got] - np.sort(T[b, rows])[:kk]) <= E[b, got] + worst).all(), (what, k, b, 'rank')
                assert (np.abs(d[b, :kk].astype(np.float64) - T[b, got]) <= E[b, got]).all(), (what, k, b, 'distance')

    judge(np.ones(len(x), bool), 'all')
    if (metric, D) == (1, 40):  # deletes plus indices=
        dead, keep = rs.choice(len(x), len(x) // 3, replace=False), rs.choice(len(x), len(x) // 2, replace=False)
        idx.delete(dead.tolist())
        live = np.zeros(len(x), bool)
        live[np.setdiff1d(keep, dead)] = True
        judge(live, 'deleted, indices', indices=keep)


@pytest.mark.parametrize('metric', [1, 2, 3])
def test_same_bits_as_the_f32_cell_index_over_the_decoded_rows(ops, metric):
    C, D, P = len(SIZES), 40, 3
    rs = np.random.RandomState(30 + metric)
    x, cell = _rows(rs, SIZES, D)
    q = _queries(rs, C, D, 130)
    new, ref, sync = _pair(ops, metric, D, _vq(C, D, metric), x, n_probe=P, expand_step_size=1024)

    def compare(what):
        _same(new.search_batch(q, limit=10), ref.search_batch(q, limit=10), (what, 10))
        assert new.last_cell_filter == 'i8x3' and new.last_overflowed == 0 and ref.last_overflowed == 0
        for large_k in ('host', 'wide'):
            _same(new.search_batch(q, limit=100, large_k=large_k), ref.search_batch(q, limit=100, large_k=large_k), (what, 100, large_k))
            assert new.last_large_k == large_k

    compare('added')
    ids = np.flatnonzero(cell == 3)[:50]
    moved = (_centroids(C, D)[4] + 0.3 * rs.randn(50, D)).astype(F)  # rows of cell 3 become rows of cell 4
    more = (_centroids(C, D)[1] + 0.3 * rs.randn(700, D)).astype(F)  # ... and the one-row cell grows past the store's capacity
    for idx, r in ((new, lambda a: a), (ref, lambda a: dec(_pre(metric, a), new.int8_scale_))):
        idx.update_with_ids(r(moved), ids)
        idx.add_with_ids(r(more), np.arange(len(x), len(x) + 700))
    sync()
    assert metric == 3 or (new._cell_of[ids].cpu().numpy() == 4).all()
    compare('updated, added again')


@pytest.fixture(params=[64, 128])  # both stages: the one the library launches and the one behind its A/B switch
def stage_depth(request, monkeypatch):
    from annlite_amd import _capi

    monkeypatch.setenv('ANNLITE_IVF_I8_STAGE', str(request.param))
    _capi.knobs_reload()  # (the library reads its switches when it is told to)
    yield request.param
    monkeypatch.delenv('ANNLITE_IVF_I8_STAGE')
    _capi.knobs_reload()


@pytest.mark.parametrize('stride', [1, 3])
@pytest.mark.parametrize('D', [5, 96])
def test_the_stage_alone_lists_every_row_within_the_bound(ops, stage_depth, D, stride):
    import torch

    sizes, P, B, k, s = [1, 127, 128, 129], 2, 40, 10, 2.0 ** -3
    C, N = len(sizes), sum(sizes)
    rs = np.random.RandomState(D + stride)
    x, q = _rows(rs, sizes, D)[0], _queries(rs, C, D, B)
    # the queries' integers Q = rne(q 2^(20 - ex)) have all three digits non-zero: the recombination's weights 2^14 / 2^7 / 1 count
    Q = np.rint(q.astype(np.float64) * 2.0 ** (20 - np.frexp(np.abs(q).max(1))[1])[:, None]).astype(np.int64)
    assert all((d != 0).mean() > 0.75 for d in _digits(Q))
    for metric in (1, 2):
        idx = _index(metric, D, _vq(C, D, metric), x, ivf_rows='i8', int8_scale=s, n_probe=P)
        idx.delete(np.arange(5, N, 9).tolist())
        idx._seal()
        qd = idx._pre(q)
        cells = idx.probe_cells(qd, P)
        perm, ranges = idx._perm.cpu().numpy(), idx._cell_rows.cpu().numpy()
        at = np.zeros((B, N), bool)  # the pairs the stage evaluates: live rows of the probed cells, every stride-th of each cell
        for b, cs in enumerate(cells.cpu().numpy()):
            for c in cs:
                at[b, perm[ranges[c, 0]:ranges[c, 1]:stride]] = True
        x64, q64 = dec(x, s).astype(np.float64), q.astype(np.float64)
        d64 = ((x64[None] - q64[:, None]) ** 2).sum(-1) if metric == 1 else 1.0 - q64 @ x64.T
        bound = np.sort(np.where(at, d64, np.inf), axis=1)[:, k - 1].astype(F)
        out = ops.ivf_flat_filter_i8(metric, qd, idx._vectors, idx._norms, ops.to_dev(bound), s, cells, C, idx._perm, idx._cell_rows,
                                     idx._cell_order, int(idx._sizes_cum[0]), valid_bits=idx._valid, n_rows=N, stride=stride, scores=True)
        torch.cuda.synchronize()
        cand, count, qn, qs, scores = (t.cpu().numpy() for t in out)
        c_rel, c_abs = ops.flat_i8_slack(metric, D)
        slack = c_rel * ((x64 ** 2).sum(1)[None, :] + (q64 ** 2).sum(1)[:, None]) + c_abs + qs[:, None].astype(np.float64)
        assert np.array_equal(~np.isnan(scores), at), 'scored: exactly the live rows of the probed cells at the stride'
        assert (np.abs(scores.astype(np.float64) - d64)[at] <= slack[at]).all(), (metric, float((np.abs(scores - d64) / slack)[at].max()))
        assert (count <= ops.flat_list_capacity()).all()  # no list overflowed: 385 rows against 4096
        for b in range(B):
            lst = cand[b, :count[b]]
            assert len(set(lst.tolist())) == len(lst) and at[b, lst].all(), (metric, b, 'a row twice, dead, or outside the probed cells')
            assert np.isin(np.flatnonzero(at[b] & (d64[b] <= bound[b])), lst).all(), (metric, b, 'a row within the bound is missing')


@pytest.mark.parametrize('metric', [1, 2])
def test_non_finite_and_zero_queries_saturated_and_zero_rows_and_dump_load(ops, metric, tmp_path):
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex

    C, D, P, s = 4, 32, 2, SCALE[metric]
    rs = np.random.RandomState(41)
    x, cell = _rows(rs, [4500, 3000, 2000, 40], D)
    far, tiny = np.flatnonzero(cell == 3)[:2], np.flatnonzero(cell == 0)[:3]
    x[far[0]], x[far[1]] = 100.0, -100.0  # beyond +-127 s: stored as +-127
    x[tiny] = 0.01                        # below s / 2: rows of all-zero codes
    q = _queries(rs, C, D, 9)
    q[1, 3], q[2, 0], q[4, :], q[6, 10] = np.inf, -np.inf, np.nan, np.nan  # qslack = +inf: the all-rows route, NaN-last order
    q[7] = 0.0                                                            # an all-zero query: planes and slack 0
    vq = _vq(C, D, metric)
    new, ref, _ = _pair(ops, metric, D, vq, x, n_probe=P)
    stored = new._vectors.cpu().numpy()
    assert (stored[far[0]] == 127).all() and (stored[far[1]] == -127).all() and not stored[tiny].any()
    for k in (10, 64):
        want = new.search_batch(q, limit=k)
        _same(want, ref.search_batch(q, limit=k), (metric, k))
    new.dump(tmp_path / 'i8.idx'), ref.dump(tmp_path / 'f32.idx')
    assert np.load(tmp_path / 'i8.idx', allow_pickle=True)[0]['vectors'].dtype == I8
    for file in ('i8.idx', 'f32.idx'):  # (the f32 file holds the decoded rows and their cells: it quantises into the same index)
        back = IvfFlatGpuIndex(D, vq_codec=vq, n_probe=P, metric=new.metric, ivf_rows='i8', int8_scale=s, index_file=tmp_path / file)
        assert back._vectors.dtype == new._vectors.dtype and back.size == new.size
        _same(back.search_batch(q, limit=64), want, file)
        assert back.last_cell_filter == 'i8x3'
