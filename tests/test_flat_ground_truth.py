"""Float search against float64: every row store, metric and way of applying a selection of ``FlatGpuIndex``, judged
by numpy float64 distances over what the index holds -- not by another search of this project.  The other flat-search files compare two
pieces of this library bit for bit (grouped with per-group, ``'rows'`` with ``'mask'``, a narrow store with the f32 index, the f32 index
with ``rerank_topk``); a defect on the path they share -- tile prologue / epilogue / launcher, sample and bound, ``flat_exact_kernel``, the
live bitmap ANDed into a selection, ``_pre`` -- passes all of them.  Here nothing in the truth calls a distance or top-k kernel.

The truth.  Rows: ``idx._vectors`` read back and widened (int8: times the scale).  Queries: what ``idx._pre`` returns.  EUCLIDEAN:
sqrt(sum (x_j - q_j)^2), the direct difference; INNER_PRODUCT, COSINE: 1 - sum x_j q_j (as test_rerank_topk.py restates them), float64.

The bound, per (query, row).  ``_refs.fp32_chain_bound`` over the terms (x_j - q_j)^2 or x_j q_j: (2 D + 4) u sum|t_j| + u |d|, u = 2^-24.
DESIGN.md section 3.6 states gamma(ceil(D / 64) + 8) sum|t_j| for the exact chain (plus the rounding u |d| of 1 - s); at D = 5 that is 9 u
against 14 u, at D = 96 it is 10 u against 196 u: the chain bound is the larger for every metric and both are computed, the maximum
taken.  EUCLIDEAN returns fl(sqrt(d^)): with |d^ - d| <= e the root moves by at most max(sqrt(d + e) - sqrt(d), sqrt(d) - sqrt(max(d - e,
0))), and the f32 square root adds at most one ulp, 2 u sqrt(d + e).  A row equal to the query has d = 0 and e = 0: it must come back at
exactly 0.0.

Judging.  A query is decided when its k-th and (k + 1)-th truths lie further apart than the sum of their two bounds (or when its selection
holds at most k live rows): its returned id set must be the truth's.  For every query: each distance within its bound of the truth of
the returned id, ids unique, live and selected, distances non-decreasing, the places past the selection's size (+inf, -1).  At most 2 % of
a search's queries may be undecided -- asserted, per search.  Every case prints its largest undecided share and its worst
|returned - truth| / bound."""
import numpy as np
import pytest

from _refs import fp32_chain_bound
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

F = np.float32
U = 2.0 ** -24
N, B, G = 9000, 130, 6  # one filter stage (above FILTER_MIN_ROWS); two query tiles, the second nearly empty
PLANT = 100             # the row query 0 is equal to
TIES = np.arange(100, 140)
MAX_UNDECIDED = 0.02    # (test_flat_search.py's share)
SEED = 0                # (of every world: the shares of undecided queries depend on the truth alone, and were checked without a GPU)
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


def _index(metric, D, x, **kw):
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.enums import Metric

    idx = FlatGpuIndex(D, metric=Metric(metric), initial_size=max(len(x), 1), **kw)
    idx.add_with_ids(x, np.arange(len(x)))
    return idx


def _words(offsets, n_rows):
    bits = np.zeros((n_rows + 31) // 32 * 32, dtype=bool)
    bits[offsets] = True
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder='little').view(np.uint32).reshape(-1).view(np.int32)


def _mask(ops, offsets, n_rows):
    """the selection as a ``RowMask``: what a filter evaluated on the device hands the index"""
    import torch
    from annlite_amd.columns import RowMask

    return RowMask(ops.to_dev(_words(offsets, n_rows)), torch.tensor([len(offsets)]), n_rows)


def _vectors(rs, metric, D, int8):
    """``draw(count, queries)`` -> f64 [count, D]: vectors whose neighbours the bound can tell apart.

    I.i.d. normal vectors are not such a world at D = 96: distances concentrate, and the 64th and 65th of 9000 rows lie closer than
    2 (2 D + 4) u sum|t_j| for 2 to 5 % of the queries (measured on the float64 truth alone): above the cap.  The share of undecided
    queries is the density of the truth at rank k times the bound, so these worlds spread the near neighbours out.

    * EUCLIDEAN, INNER_PRODUCT: points of a random 2-dimensional subspace (every coordinate takes part) with log-normal lengths,
      exp(2 * normal), plus a little noise of full rank.  In 2 dimensions the k-th and (k + 1)-th distance differ by about 1 / (2 k) of
      themselves, against a bound of 196 u of them; the heavy-tailed lengths do the same for the largest inner products.  int8 rows
      have seven bits for the lengths (exp(0.5 * normal)) and need noise of two code steps, or rows of the subspace share their codes.
    * COSINE: the bound is absolute -- sum|x_j q_j| of unit vectors -- so neighbours at small angles are never told apart.  Rows are of
      unit size on all coordinates but three, where they carry a small part of log-normal size; queries live on those three (the
      first, the middle, the last) with a few percent of their length elsewhere.  The cosines are small, heavy-tailed multiples of
      that shared part and sum|x_j q_j| is about |cos|: the bound scales with the distance again.  Every coordinate still moves every
      distance by more than its bound.  int8 rows (codes of 1 / 64) need a larger shared part to resolve it."""
    if metric == 3:
        a = np.array([0, D // 2, D - 1])
        b = np.setdiff1d(np.arange(D), a)
        small, spread, beside = (0.1, 1.0, 0.1) if int8 else (0.005, 2.0, 0.03)

        def draw(count, queries):
            v = np.empty((count, D))
            if queries:
                v[:, a], v[:, b] = rs.randn(count, 3), beside * rs.randn(count, len(b)) / np.sqrt(len(b))
            else:
                v[:, b] = rs.randn(count, len(b)) / np.sqrt(len(b))
                v[:, a] = (small * np.exp(spread * rs.randn(count)))[:, None] * rs.randn(count, 3)
            return v
    else:
        basis = np.linalg.qr(rs.randn(D, 2))[0].T * np.sqrt(D / 2)
        spread, noise = (0.5, 0.1) if int8 else (2.0, 0.02)

        def draw(count, queries):
            return (np.exp(spread * rs.randn(count))[:, None] * rs.randn(count, 2)) @ basis + noise * rs.randn(count, D)
    return draw


def _world(D, kind, metric, n=N, nq=B, ties=False):
    """rows, queries and the deleted rows.  Row ``plant`` is a row scaled to small integers -- every store holds them as they are -- and
    query 0 equals it.  ``ties``: the forty rows TIES equal it, and so does query 1."""
    rs = np.random.RandomState(1000 * D + 10 * len(kind) + metric + n + SEED)
    scale = 10 if kind == 'i8' else 1  # (int8 codes are steps of 0.5; COSINE: of 1 / 64, after normalising)
    offset = 50 if kind == 'bf16x3' and metric == 1 else 0  # a common offset -- what the centre is for, and the centre is EUCLIDEAN's
    draw = _vectors(rs, metric, D, kind == 'i8')
    x, q = (draw(n, False) * scale + offset).astype(F), (draw(nq, True) * scale + offset).astype(F)
    plant = min(PLANT, n - 2)
    x[plant] = np.rint((x[plant] - offset) * (8 / np.abs(x[plant] - offset).max())) + offset
    if ties:
        # (the block is one of the longest rows in a hundred: out where rows are sparse, so that few other queries find it near their
        # k-th place -- forty equal truths decide nothing there --, and inside the subspace, so that its own neighbours are told apart)
        far = x[np.argsort(np.linalg.norm(x - offset, axis=1))[-len(x) // 100]] - offset
        x[plant] = np.clip(np.rint(far), *((-63, 63) if kind == 'i8' else (-2048, 2048))) + offset
        x[TIES] = q[1] = x[plant]
    q[0] = x[plant]
    keep = np.concatenate([TIES if ties else [plant], [31, 32, 63, 64, n - 1]])
    gone = np.setdiff1d(rs.permutation(n)[:50 if n >= 1000 else 5], keep)  # about 50 deleted rows
    return rs, x, q, gone, plant


# ---- the truth (numpy float64 only) ----------------------------------------------------------------------------------------------------
def _stored(idx):
    v = idx._vectors[:idx._n_rows].cpu().numpy().astype(np.float64)
    return v * idx.int8_scale_ if idx.int8_scale_ else v


def _truth(metric, x64, q64):
    """``(T, E)`` f64 [B, N]: the distance the index reports for (query, row) in float64 and the bound on |reported - T| (module
    docstring)."""
    D = x64.shape[1]
    T, E = np.empty((len(q64), len(x64))), np.empty((len(q64), len(x64)))
    gamma = 1.01 * (-(-D // 64) + 8) * U  # (the exact chain)
    for b, qb in enumerate(q64):
        terms = (x64 - qb) ** 2 if metric == 1 else x64 * qb
        d = terms.sum(1) if metric == 1 else 1.0 - terms.sum(1)
        e = np.maximum(fp32_chain_bound(terms, d, D), gamma * np.abs(terms).sum(1) + U * np.abs(d))
        if metric == 1:
            root = np.sqrt(d)
            e = np.maximum(np.sqrt(d + e) - root, root - np.sqrt(np.maximum(d - e, 0.0))) + 2.0 * U * np.sqrt(d + e)
            d = root
        T[b], E[b] = d, e
    return T, E


def _ranked(T, E, at, rows, kmax=65):
    """For the queries ``at`` over the rows ``rows`` (ascending): the first ``kmax`` rows by truth, their truths and their bounds."""
    Ts = T[np.ix_(at, rows)]
    order = np.argsort(Ts, axis=1, kind='stable')[:, :kmax]
    r = rows[order]
    return r, np.take_along_axis(Ts, order, axis=1), E[at[:, None], r]


def _decided(ranked, k):
    """bool per query: the k-th and (k + 1)-th truths are further apart than their two bounds (or there is no (k + 1)-th)"""
    r, t, e = ranked
    if r.shape[1] <= k:
        return np.ones(len(r), bool)
    return t[:, k] - t[:, k - 1] > e[:, k] + e[:, k - 1]


class _Stats:
    def __init__(self):
        self.undecided, self.ratio = 0.0, 0.0

    def line(self, what):
        return f'ground truth {what}: largest undecided share {self.undecided:.4f}, worst |returned - truth| / bound {self.ratio:.4f}'


def _judge(T, E, at, rows, ranked, d, i, k, what, stats):
    """The answer ``(d, i)`` [len(at), k] for the queries ``at``, whose selection's live rows are ``rows``; returns how many are undecided."""
    assert d.dtype == np.float32 and i.dtype == np.int64 and d.shape == i.shape == (len(at), k), what
    kk = min(k, len(rows))
    assert (i[:, kk:] == -1).all() and np.isposinf(d[:, kk:]).all(), (what, 'places past the selection')
    assert (d[:, 1:] >= d[:, :-1]).all(), (what, 'order')  # (no NaN in these worlds; +inf >= +inf)
    if kk == 0:
        return 0
    got = i[:, :kk]
    assert np.isin(got, rows).all(), (what, 'a row that is deleted or not selected', got[~np.isin(got, rows)][:5])
    by_id = np.sort(got, axis=1)
    assert (by_id[:, 1:] != by_id[:, :-1]).all(), (what, 'a row twice')
    t, e = T[at[:, None], got], E[at[:, None], got]
    err = np.abs(d[:, :kk].astype(np.float64) - t)
    assert (err <= e).all(), (what, 'distance', np.argwhere(err > e)[:5], err[err > e][:5], e[err > e][:5])
    stats.ratio = max(stats.ratio, float((err[e > 0] / e[e > 0]).max()) if (e > 0).any() else 0.0)
    decided = _decided(ranked, k)
    want = np.sort(ranked[0][:, :kk], axis=1)
    wrong = decided & (by_id != want).any(axis=1)
    assert not wrong.any(), (what, 'not the nearest', at[wrong][:5], by_id[wrong][:2], want[wrong][:2])
    return int((~decided).sum())


def _cap(undecided, n_queries, what, stats):
    stats.undecided = max(stats.undecided, undecided / n_queries)
    assert undecided / n_queries <= MAX_UNDECIDED, (what, undecided, n_queries)


def _battery(ops, idx, tag, q, gone, plant, rs, stats, what, ks=(1, 10, 64)):
    """Every way of searching the index, judged.  ``tag``: the filter a table scan must report (None: the table is below the filter)."""
    n, nq = idx._n_rows, len(q)
    T, E = _truth(int(idx.metric), _stored(idx), idx._pre(q).cpu().numpy().astype(np.float64))
    every, live = np.arange(nq), np.setdiff1d(np.arange(n), gone)
    half = np.union1d(np.flatnonzero(rs.rand(n) < 0.5), TIES if plant is None else [plant])
    tenth = np.union1d(np.flatnonzero(rs.rand(n) < 0.1), np.array([] if plant is None else [plant], np.int64))
    special = np.unique([r for r in (31, 32, 63, 64, n - 1) if r < n] + [gone[0]])
    group_of = every % G
    at_of = [np.flatnonzero(group_of == g) for g in range(G)]
    half_live, tenth_live = np.intersect1d(half, live), np.intersect1d(tenth, live)
    r_live, r_half, r_tenth = _ranked(T, E, every, live), _ranked(T, E, every, half_live), _ranked(T, E, every, tenth_live)

    def list_filter(rows):  # what last_flat_filter reports after a 'rows' search over ``rows``
        return tag if tag and len(rows) >= idx.FILTER_MIN_ROWS else None

    def single(k, indices, rows, ranked, route, name):
        d, i = idx.search_batch(q, limit=k, indices=indices, filter_route=route)
        w = (what, name, route, k)
        assert idx.last_filter_route == route, w
        assert idx.last_flat_filter == (tag if route == 'mask' else list_filter(rows)), (w, idx.last_flat_filter)
        assert idx.last_overflowed == 0, w
        _cap(_judge(T, E, every, rows, ranked, d, i, k, w, stats), nq, w, stats)
        return d, i

    answers = {}
    for k in ks:
        for route in ('mask', 'rows'):  # (deleted rows: there is something to compact)
            answers[k, 'all', route] = single(k, None, live, r_live, route, 'all')
            answers[k, 'tenth', route] = single(k, tenth, tenth_live, r_tenth, route, 'tenth as offsets')
            single(k, _mask(ops, tenth, n), tenth_live, r_tenth, route, 'tenth as a RowMask')
            # (at N = 9000 the half holds more than 4096 live rows: the 'rows' route runs its filter over the list, the tenth does not)
            answers[k, 'half', route] = single(k, _mask(ops, half, n), half_live, r_half, route, 'half as a RowMask')
        few = np.sort(rs.permutation(live)[:k - 1])
        sels = [None, _mask(ops, half, n), tenth, few, np.zeros(0, np.int64), special]
        rows_of = [live, half_live, tenth_live, few, few[:0], np.intersect1d(special, live)]
        assert len(rows_of[5]) == len(special) - 1
        d, i = idx.search_batch_grouped(q, limit=k, selections=sels, group_of=group_of)
        w = (what, 'grouped', k)
        assert idx.last_filter_batch == 'grouped' and idx.last_filter_route == 'mask' and idx.last_flat_filter == tag, w
        assert idx.last_overflowed == 0, w
        undecided = 0
        for g in range(G):
            at = at_of[g]
            ranked = [r_live, r_half, r_tenth][g] if g < 3 else _ranked(T, E, every, rows_of[g])
            undecided += _judge(T, E, at, rows_of[g], tuple(a[at] for a in ranked), d[at], i[at], k, (w, g), stats)
        _cap(undecided, nq, w, stats)
        answers[k, 'grouped'] = d, i
        if plant is not None and int(idx.metric) == 1:  # a stored row searched with itself: 0.0, first
            for dd, ii in (answers[k, 'all', 'mask'], answers[k, 'tenth', 'rows'], answers[k, 'grouped']):
                assert dd[0, 0] == 0.0 and ii[0, 0] == plant, (what, k)
    return answers


# ---- 1. the matrix ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [5, 96])  # scalar staging and the vector path
@pytest.mark.parametrize('metric', [1, 2, 3])
@pytest.mark.parametrize('kind', list(KINDS))
def test_search_returns_the_float64_nearest(ops, kind, metric, D):
    """N = 9000 (a filter stage runs), 130 queries, about 50 deleted rows, k = 1, 10, 64: no selection, a tenth as offsets and as a
    ``RowMask``, a half as a ``RowMask`` -- each on the ``'mask'`` and the ``'rows'`` route -- and six selections in one grouped launch.  The
    bound is ``fp32_chain_bound``: for every metric it is larger than DESIGN.md's gamma(ceil(D / 64) + 8) (module docstring)."""
    kw, tag = KINDS[kind]
    rs, x, q, gone, plant = _world(D, kind, metric)
    idx = _index(metric, D, x, **kw(metric))
    idx.delete(gone)
    stats = _Stats()
    _battery(ops, idx, tag, q, gone, plant, rs, stats, (kind, metric, D))
    print(stats.line(f'{kind} metric {metric} D {D}'))


# ---- 2. a table below the filter: flat_exact_kernel alone ------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [63, 4096])
@pytest.mark.parametrize('metric', [1, 2, 3])
@pytest.mark.parametrize('kind', ['f32', 'i8'])
def test_a_table_below_the_filter(ops, kind, metric, n):
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex

    assert n < FlatGpuIndex.FILTER_MIN_ROWS
    stats = _Stats()
    for D in (5, 96):
        rs, x, q, gone, plant = _world(D, kind, metric, n=n)
        idx = _index(metric, D, x, **KINDS[kind][0](metric))
        idx.delete(gone)
        _battery(ops, idx, None, q, gone, plant, rs, stats, (kind, metric, D, n))  # (None: last_flat_filter reports that no filter ran)
    print(stats.line(f'{kind} metric {metric} N {n}'))


# ---- 3. ties ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', list(KINDS))
def test_identical_rows_come_back_in_id_order(ops, kind):
    """Forty identical rows inside the half mask and a query equal to them, EUCLIDEAN, k = 64: on the masked scan, the compacted list and
    the grouped launch the first forty places are those rows in ascending id order at 0.0 (their truth and bound are 0: the order among
    them is the documented (distance, id) order); the other 24 are judged by the truth."""
    kw, tag = KINDS[kind]
    D, k = 96, 64
    rs, x, q, gone, _ = _world(D, kind, 1, ties=True)
    idx = _index(1, D, x, **kw(1))
    idx.delete(gone)
    stats = _Stats()
    answers = _battery(ops, idx, tag, q, gone, None, rs, stats, (kind, 'ties'), ks=(k,))
    assert len(np.intersect1d(TIES, gone)) == 0
    # (query 1 is in group 1, the half; query 0 in group 0, no selection)
    for b, name in ((1, (k, 'half', 'mask')), (1, (k, 'half', 'rows')), (1, (k, 'grouped')), (0, (k, 'grouped')), (0, (k, 'all', 'mask'))):
        dd, ii = answers[name]
        assert list(ii[b, :len(TIES)]) == list(TIES) and (dd[b, :len(TIES)] == 0.0).all() and dd[b, len(TIES)] > 0.0, (kind, name)
    print(stats.line(f'{kind} ties'))


# ---- 4. two filter stages --------------------------------------------------------------------------------------------------------------
def test_two_filter_stages(ops):
    """N = 140 000: two filter stages, grouped masks of 50 / 10 / 1 % -- the last keeps about 40 of the 4096 sampled rows, so k = 10 still
    gets a finite first bound.  The truth per group."""
    rs = np.random.RandomState(5)
    n, D, nq, k = 140_000, 16, 64, 10
    x, q = rs.randn(n, D).astype(F), rs.randn(nq, D).astype(F)
    idx = _index(1, D, x)
    T, E = _truth(1, _stored(idx), idx._pre(q).cpu().numpy().astype(np.float64))
    rows_of = [np.flatnonzero(rs.rand(n) < p) for p in (0.5, 0.1, 0.01)]
    group_of = np.arange(nq) % 3
    d, i = idx.search_batch_grouped(q, limit=k, selections=[_mask(ops, r, n) for r in rows_of], group_of=group_of)
    assert idx.last_filter_batch == 'grouped' and idx.last_flat_filter == 'f32' and idx.last_filter_route == 'mask'
    assert idx.last_overflowed == 0
    stats, undecided = _Stats(), 0
    for g, rows in enumerate(rows_of):
        at = np.flatnonzero(group_of == g)
        undecided += _judge(T, E, at, rows, _ranked(T, E, at, rows), d[at], i[at], k, ('two stages', g), stats)
    _cap(undecided, nq, 'two stages', stats)
    print(stats.line('f32 metric 1 N 140000'))
