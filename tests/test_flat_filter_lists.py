"""The candidate lists of the float filters, pinned EXACTLY (``flat.hip``).

The stage tests of ``test_flat_*_search`` / ``test_ivf_flat_split_search`` are one-sided: every row within the bound must be listed.
Here the data make every filter's arithmetic exact -- rows and queries are small integers, so the f32, split-bf16, f16 and int8
contractions, the norms and the scores are all integers far below 2^24 -- and each bound sits half a unit away from every score.  The
test first asserts (in numpy, with the slack terms the entry points themselves report) that no score lies within the slack of its
bound: a condition on the inputs, not a tolerance.  Then the listed set of every query is one known set, whichever kernel made it.

Shapes: 900 rows at stride 3 (two full row tiles and one of 44) and stride 1; 130 queries (a full query tile and one of 2); D = 5
(scalar staging, a partial K step), 48 (vector staging of every kernel, a partial LDS stage) and 96 (three stages of 32; int8: 64 + 32);
one row in seven cleared in the bitmap, rows of the last, partial tile among them."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

F = np.float32
EUCLIDEAN, INNER_PRODUCT = 1, 2
N, B, K = 900, 130, 10
DIMS = [5, 48, 96]
STRIDES = [3, 1]
TABLE_CASES = [('f32', EUCLIDEAN), ('f32', INNER_PRODUCT), ('split', EUCLIDEAN), ('split', INNER_PRODUCT), ('split_centred', EUCLIDEAN),
               ('f16', EUCLIDEAN), ('f16', INNER_PRODUCT), ('i8', EUCLIDEAN), ('i8', INNER_PRODUCT)]


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _bitmap(ops, ok):
    import torch
    from annlite_amd.core.index.row_store import RowStoreIndex

    flags = torch.zeros(((len(ok) + 31) // 32 + 2) * 32, dtype=torch.bool)
    flags[:len(ok)] = torch.tensor(ok)
    return RowStoreIndex._pack_bits(flags.to(ops.device()))


_DATA = {}


def _data(D):
    """(x i64 [N, D], q i64 [B, D], centre i64 [D], ok bool [N]) -- computed once per D and never written to"""
    if D not in _DATA:
        rs = np.random.RandomState(1000 + D)
        x = rs.randint(-4, 5, size=(N, D)).astype(np.int64)
        q = rs.randint(-4, 5, size=(B, D)).astype(np.int64)
        centre = rs.randint(-2, 3, size=D).astype(np.int64)
        ok = np.ones(N, bool)
        ok[3::7] = False
        for stride in STRIDES:  # a cleared stage row in the last, partial row tile
            S = (N + stride - 1) // stride
            last = np.arange(S // 128 * 128, S) * stride
            assert S % 128 and (~ok[last]).any() and ok[last].any()
        for a in (x, q, centre, ok):
            a.setflags(write=False)
        _DATA[D] = (x, q, centre, ok)
    return _DATA[D]


def _integer_scores(metric, x, q, centre, ok):
    """(v i64 [B, N], a i64 [B, N]): the filter's score and its a = |x|^2 + |q|^2 over the values it contracts (centred where a
    centre is given); a row that is not valid has |x|^2 = 0 there, as the kernels hold it."""
    xc, qc = x - centre[..., None, :], q - centre[..., None, :]
    nx = np.where(ok, (xc * xc).sum(-1), 0)
    a = nx + (qc * qc).sum(-1)[..., :, None]
    dot = np.einsum('...bd,...nd->...bn', qc, xc)
    return (a - 2 * dot if metric == EUCLIDEAN else 1 - dot), a


def _bounds(v, rows_ok):
    """per query: the K-th smallest score among the valid stage rows, plus one half"""
    return (np.sort(np.where(rows_ok, v, np.iinfo(np.int64).max), axis=1)[:, K - 1] + 0.5).astype(F)


def _assert_clear_of_the_slack(v, a, bound, c_rel, c_abs, extra, where):
    slack = (F(c_rel) * a.astype(F) + F(c_abs)).astype(np.float64) + (0.0 if extra is None else extra.astype(np.float64)[:, None])
    gap = np.abs(v.astype(np.float64) - bound.astype(np.float64)[:, None])
    assert np.isfinite(slack).all() and (gap[:, where] > 2.0 * slack[:, where]).all(), 'a score within (twice) the slack of its bound'
    return float((slack[:, where] / gap[:, where]).max())


def _assert_lists(cand, count, want, what):
    for b in range(len(want)):
        exp = np.flatnonzero(want[b])
        assert count[b] == len(exp), (what, b, int(count[b]), len(exp))
        got = cand[b, :count[b]]
        assert len(set(got.tolist())) == len(got) and np.array_equal(np.sort(got), exp), (what, b)


def _table_entry(ops, kind, metric, D, stride, x, q, centre, ok, bound, scores=True):
    """-> (cand, count, scores or None, (c_rel, c_abs), per-query extra slack or None), all numpy"""
    import torch

    qd, bd, bits = ops.to_dev(q.astype(F)), ops.to_dev(bound), _bitmap(ops, ok)
    kw = dict(valid_bits=bits, stride=stride)
    extra = sc = None
    if kind == 'f32':
        xd = ops.to_dev(x.astype(F))
        cand, count = ops.flat_filter(metric, qd, xd, ops.flat_row_norms(xd), bd, **kw)
        slack = ops.flat_slack(metric, D)
    elif kind in ('split', 'split_centred'):
        xd = ops.to_dev(x.astype(F))
        mu = ops.to_dev(centre.astype(F)) if kind == 'split_centred' else None
        norms = ops.flat_centred_norms(xd, mu) if mu is not None else ops.flat_row_norms(xd)
        cand, count, _, *rest = ops.flat_filter_split(metric, qd, xd, norms, bd, centre=mu, scores=scores, **kw)
        sc = rest[0] if scores else None
        slack = ops.flat_split_slack(metric, D)
    elif kind == 'f16':
        xd = ops.to_dev(x.astype(np.float16))
        cand, count, _, extra, *rest = ops.flat_filter_f16(metric, qd, xd, ops.flat_row_norms_f16(xd), bd, scores=scores, **kw)
        sc = rest[0] if scores else None
        slack = ops.flat_f16_slack(metric, D)
    else:
        xd = ops.to_dev(x.astype(np.int8))
        cand, count, _, extra, *rest = ops.flat_filter_i8(metric, qd, xd, ops.flat_row_norms_i8(xd, 1.0), bd, 1.0, scores=scores, **kw)
        sc = rest[0] if scores else None
        slack = ops.flat_i8_slack(metric, D)
    torch.cuda.synchronize()
    cpu = lambda t: None if t is None else t.cpu().numpy()
    return cpu(cand), cpu(count), cpu(sc), slack, cpu(extra)


# ---- 1. the table filters ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,metric', TABLE_CASES)
@pytest.mark.parametrize('D', DIMS)
def test_table_filter_lists_exactly_the_rows_below_the_bound(ops, D, kind, metric):
    x, q, centre, ok = _data(D)
    mu = centre if kind == 'split_centred' else np.zeros(D, np.int64)
    v, a = _integer_scores(metric, x, q, mu, ok)
    for stride in STRIDES:
        stage = np.zeros(N, bool)
        stage[::stride] = True
        live = stage & ok
        bound = _bounds(v, live)
        cand, count, sc, (c_rel, c_abs), extra = _table_entry(ops, kind, metric, D, stride, x, q, mu, ok, bound)
        worst = _assert_clear_of_the_slack(v, a, bound, c_rel, c_abs, extra, live)
        print(f'{kind} D={D} metric={metric} stride={stride}: slack / gap <= {worst:.4f}')
        want = live[None, :] & (v < bound[:, None])
        assert (want.sum(axis=1) >= K).all()
        _assert_lists(cand, count, want, (kind, D, metric, stride))
        if kind != 'f32':  # (the f32 entry has no scores output)
            assert sc.shape == (B, (N + stride - 1) // stride)
            assert np.array_equal(sc, v[:, ::stride].astype(F)), 'scores differ from the integer scores'


# ---- 2. the split filter over cell tiles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric,centred', [(EUCLIDEAN, False), (EUCLIDEAN, True), (INNER_PRODUCT, False)])
@pytest.mark.parametrize('D', DIMS)
def test_cell_filter_lists_exactly_the_rows_below_the_bound(ops, D, metric, centred):
    import torch

    x, q, _, ok = _data(D)
    sizes, C, P = [600, 300], 2, 2
    rs = np.random.RandomState(7 * D + metric)
    cell = rs.permutation(np.repeat(np.arange(C), sizes))
    cells = np.stack([np.arange(B) % C, (np.arange(B) + 1) % C], axis=1).astype(np.int32)  # every query probes both, either order
    perm = np.argsort(cell, kind='stable').astype(np.int32)
    end = np.cumsum(sizes)
    cell_rows = np.stack([end - sizes, end], axis=1).astype(np.int64)
    cell_order = np.argsort(-np.asarray(sizes), kind='stable').astype(np.int32)
    cent = rs.randint(-2, 3, size=(C, D)).astype(np.int64) if centred else np.zeros((C, D), np.int64)
    # a row and a query are centred on the row's cell: the score of the pair is over those values
    v = np.empty((B, N), np.int64)
    a = np.empty((B, N), np.int64)
    for c in range(C):
        m = cell == c
        v[:, m], a[:, m] = _integer_scores(metric, x[m], q, cent[c], ok[m])
    xd, qd = ops.to_dev(x.astype(F)), ops.to_dev(q.astype(F))
    cell_of = ops.to_dev(cell.astype(np.int32))
    centres = ops.to_dev(cent.astype(F)) if centred else None
    norms = ops.ivf_flat_centred_norms(xd, centres, cell_of) if centred else ops.flat_row_norms(xd)
    bits = _bitmap(ops, ok)
    c_rel, c_abs = ops.flat_split_slack(metric, D)
    for stride in STRIDES:
        stage = np.zeros(N, bool)
        for b0, e0 in cell_rows:
            stage[perm[b0:e0:stride]] = True  # every stride-th entry of EACH cell's range
        live = stage & ok
        bound = _bounds(v, live)
        worst = _assert_clear_of_the_slack(v, a, bound, c_rel, c_abs, None, live)
        print(f'cells D={D} metric={metric} centred={centred} stride={stride}: slack / gap <= {worst:.4f}')
        cand, count, pn, sc = ops.ivf_flat_filter_split(metric, qd, xd, norms, ops.to_dev(bound), ops.to_dev(cells), C, ops.to_dev(perm),
                                                        ops.to_dev(cell_rows), ops.to_dev(cell_order), max(sizes), centres=centres,
                                                        cell_of=cell_of if centred else None, valid_bits=bits, stride=stride, scores=True)
        torch.cuda.synchronize()
        cand, count, sc = cand.cpu().numpy(), count.cpu().numpy(), sc.cpu().numpy()
        want = live[None, :] & (v < bound[:, None])
        assert (want.sum(axis=1) >= K).all()
        _assert_lists(cand, count, want, ('cells', D, metric, centred, stride))
        assert sc.shape == (B, N) and np.isnan(sc[:, ~live]).all()  # (not evaluated: the caller's NaN)
        assert np.array_equal(sc[:, live], v[:, live].astype(F)), 'scores differ from the integer scores'


# ---- 3. an overflowed list -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['f32', 'split', 'f16', 'i8'])
def test_overflowed_list_holds_cap_distinct_valid_rows(ops, kind):
    n, D, nq = 4500, 5, 3
    rs = np.random.RandomState(77)
    x = rs.randint(-4, 5, size=(n, D)).astype(np.int64)
    q = rs.randint(-4, 5, size=(nq, D)).astype(np.int64)
    ok = np.ones(n, bool)
    ok[11::50] = False
    cap = ops.flat_list_capacity()
    assert ok.sum() > cap
    bound = np.full(nq, np.inf, F)
    cand, count, _, _, _ = _table_entry(ops, kind, EUCLIDEAN, D, 1, x, q, np.zeros(D, np.int64), ok, bound, scores=False)
    for b in range(nq):
        assert count[b] > cap  # (its value past the cap depends on the order of the atomics)
        got = cand[b]
        assert got.shape == (cap,) and len(set(got.tolist())) == cap
        assert ((got >= 0) & (got < n)).all() and ok[got].all()
