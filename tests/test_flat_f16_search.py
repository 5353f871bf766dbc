"""The half-precision row store of the exact float search on the GPU ("f16 rows"): ``dtype=np.float16``
returns, bit for bit, what the f32 index returns over the rounded rows widened back to f32; the f16 MFMA's operand map on exact
integer data; at the stage level every row within the bound is listed and the measured error stays inside the derived slack;
non-finite inputs keep the convention; update, dump / load across the dtypes and growth."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

F = np.float32
H = np.float16


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def f16(a):
    """the rows as an f16 index stores them, widened back to f32"""
    with np.errstate(over='ignore'):
        return np.asarray(a, dtype=F).astype(H).astype(F)


def _index(metric, D, x, **kw):
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.enums import Metric

    kw.setdefault('initial_size', max(len(x), 1))
    idx = FlatGpuIndex(D, metric=Metric(metric), **kw)
    idx.add_with_ids(x, np.arange(len(x)))
    return idx


def _pair(metric, D, x, q):
    """(the f16 index over x, the f32 index that holds what it stores, the queries for either).  COSINE: an INNER_PRODUCT f32 index
    over the host-normalised-then-rounded rows, asked with the host-normalised queries -- a COSINE f32 index would normalise the
    rounded rows again."""
    from annlite_amd.math import l2_normalize_host

    new = _index(metric, D, x, dtype=np.float16)
    if metric == 3:
        return new, _index(2, D, f16(l2_normalize_host(x))), l2_normalize_host(q)
    return new, _index(metric, D, f16(x)), q


def _same(got, want, what):
    (gd, gi), (wd, wi) = got, want
    assert gi.dtype == np.int64 and gd.dtype == np.float32
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:5], gi[gi != wi][:5], wi[gi != wi][:5])
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (what, 'distance bits')


# ---- the same answer, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [4097, 4225, 20000])  # the filter engages above 4096 rows; a tile is 128 rows: 1 row, 1 tile + 1, many
@pytest.mark.parametrize('D', [1, 5, 16, 33, 128, 770])
def test_f16_index_gives_the_f32_index_over_the_rounded_rows_its_bits(ops, D, N):
    import torch

    rs = np.random.RandomState(1000 * D + N % 997)
    x = rs.randn(N, D).astype(F)
    x[100:140] = x[100]  # a block of identical rows: ties ordered by id
    q = rs.randn(129, D).astype(F)
    q[0] = f16(x[100])   # a query equal to stored rows
    gone = np.arange(0, N, 3)
    keep = np.arange(1, N, 5)
    for metric in (1, 2, 3):
        new, ref, qr = _pair(metric, D, x, q)
        assert new._vectors.dtype == torch.float16 and ref._vectors.dtype == torch.float32 and new.flat_filter == 'f16x2'
        assert np.array_equal(new._vectors[:N].cpu().numpy().view(np.uint16), ref._vectors[:N].cpu().numpy().astype(H).view(np.uint16))
        for B in (1, 129):
            for k in (1, 10, 64, 100):
                got, want = new.search_batch(q[:B], limit=k), ref.search_batch(qr[:B], limit=k)
                _same(got, want, (metric, B, k))
                ran = k <= 64 or N > 2 * ops.flat_list_capacity()  # (limit > 64 on a small table: exact sums over all rows, no filter)
                assert new.last_flat_filter == ('f16x2' if ran else None) and ref.last_flat_filter == ('f32' if ran else None)
                assert new.last_overflowed == ref.last_overflowed
                # i.i.d. normal rows: no list overflows -- but for COSINE at D = 1, where every normalised row is +1 or -1: half the
                # table ties at distance 0, and where that is more than a list holds the f32 index overflows as well
                assert ref.last_overflowed == 0 or (metric, D) == (3, 1), (metric, B, k)
                if metric == 1:
                    assert got[0][0, 0] == 0.0 and got[1][0, 0] == 100 and (k < 10 or list(got[1][0, :10]) == list(range(100, 110)))
        _same(new.search_batch(q, limit=10, indices=keep), ref.search_batch(qr, limit=10, indices=keep), (metric, 'a fifth kept'))
        assert new.last_flat_filter == 'f16x2' and new.last_overflowed == ref.last_overflowed
        for idx in (ref, new):
            idx.delete(gone)
        for B, k in ((129, 10), (1, 64), (5, 100)):
            _same(new.search_batch(q[:B], limit=k), ref.search_batch(qr[:B], limit=k), (metric, B, k, 'a third deleted'))
            assert new.last_flat_filter == ('f16x2' if k <= 64 or N > 2 * ops.flat_list_capacity() else None)
            assert new.last_overflowed == ref.last_overflowed


def test_small_tables_run_no_filter(ops):
    rs = np.random.RandomState(2)
    x, q = rs.randn(4096, 16).astype(F), rs.randn(3, 16).astype(F)
    small, ref = _index(1, 16, x, dtype='float16'), _index(1, 16, f16(x))
    for k in (10, 100):
        _same(small.search_batch(q, limit=k), ref.search_batch(q, limit=k), ('4096 rows', k))
        assert small.last_flat_filter is None and small.last_overflowed == 0


# ---- the f16 MFMA's operand map: exact integer data, an asymmetric B --------------------------------------------------------------------
@pytest.mark.parametrize('D', [40, 16, 5])
def test_filter_scores_of_integer_data_are_exact(ops, D):
    import torch

    N, B = 300, 130  # (3 row tiles, 2 query tiles, both with a ragged edge; D = 40: a K step that is half padding)
    r, j, b = np.arange(N)[:, None], np.arange(D)[None, :], np.arange(B)[:, None]
    x = ((r * 7 + j * 3) % 11 - 5).astype(F)
    q = ((b * 5 + j * j + b * j) % 13 - 6).astype(F)  # (not symmetric in (row, coordinate): a swapped operand or tile shows)
    q[:, 0] = 6  # (every query's largest value: one scale, 2^12, and integer planes)
    xd, qd = ops.to_dev(x.astype(H)), ops.to_dev(q)
    norms = ops.flat_row_norms_f16(xd)
    assert np.array_equal(norms.cpu().numpy(), (x * x).sum(1))
    bound = ops.to_dev(np.full(B, np.inf, F))
    for metric in (1, 2):
        cand, count, qn, qf, scores = ops.flat_filter_f16(metric, qd, xd, norms, bound, scores=True)
        torch.cuda.synchronize()
        dot = q.astype(np.float64) @ x.astype(np.float64).T
        want = ((x * x).sum(1)[None, :] + (q * q).sum(1)[:, None] - 2 * dot) if metric == 1 else 1 - dot
        assert np.array_equal(scores.cpu().numpy(), want.astype(F)), (metric, D)
        assert np.array_equal(qn.cpu().numpy(), (q * q).sum(1)) and (count.cpu().numpy() == N).all()
        assert np.array_equal(np.sort(cand.cpu().numpy()[:, :N], axis=1), np.tile(np.arange(N, dtype=np.int32), (B, 1)))


# ---- the stage alone: a superset, and the measured error ------------------------------------------------------------------------------
def _family(name, N, D, B, rs):
    if name == 'near-duplicates':
        x = rs.randn(N, D).astype(F)
        return x, (x[:B] * F(1 + 2 ** -20) + F(1e-6) * rs.randn(B, D)).astype(F)
    if name == 'identical':
        x = rs.randn(N, D).astype(F)
        return x, f16(x[7:7 + B])
    if name == 'mixed magnitudes':
        scale = (10.0 ** rs.uniform(-3, 3, size=(1, D))).astype(F)  # (inside the f16 range)
        return (rs.randn(N, D) * scale).astype(F), (rs.randn(B, D) * scale[:, ::-1]).astype(F)
    if name == 'tiny':
        return (2e-6 * rs.randn(N, D)).astype(F), (1e-18 * rs.randn(B, D)).astype(F)  # rows: f16 subnormals
    if name == 'tiny rows, unit queries':
        return (2e-6 * rs.randn(N, D)).astype(F), rs.randn(B, D).astype(F)
    if name == 'large queries':
        return rs.randn(N, D).astype(F), (1e17 * rs.randn(B, D)).astype(F)
    assert name == 'adversarial mantissas'
    m = F(1 + 2.0 ** -11 - 2.0 ** -23)
    mk = lambda n: (m * rs.choice([-1.0, 1.0], size=(n, D)) * 2.0 ** rs.randint(-3, 4, size=(n, D))).astype(F)
    return mk(N), mk(B)


FAMILIES = ['near-duplicates', 'identical', 'mixed magnitudes', 'tiny', 'tiny rows, unit queries', 'large queries', 'adversarial mantissas']


@pytest.mark.parametrize('metric', [1, 2])
@pytest.mark.parametrize('D', [5, 128])
@pytest.mark.parametrize('family', FAMILIES)
def test_stage_lists_every_row_within_the_bound(ops, family, D, metric):
    import torch
    from annlite_amd.core.index.row_store import RowStoreIndex

    N, B, k = 4225, 8, 10
    rs = np.random.RandomState(17 * D + len(family))
    x, q = _family(family, N, D, B, rs)
    x = f16(x)
    xd, qd = ops.to_dev(x.astype(H)), ops.to_dev(q)
    flags = torch.ones(((N + 31) // 32 + 2) * 32, dtype=torch.bool, device=xd.device)
    flags[N:] = False
    flags[torch.arange(3, N, 7, device=xd.device)] = False  # (under `cap` valid rows: no list can overflow)
    bits = RowStoreIndex._pack_bits(flags)
    ok = flags[:N].cpu().numpy()
    norms = ops.flat_row_norms_f16(xd)
    assert np.array_equal(norms.cpu().numpy().view(np.uint32), ops.flat_row_norms(ops.to_dev(x)).cpu().numpy().view(np.uint32))
    rows = torch.arange(N, dtype=torch.int64, device=xd.device)[None, :].expand(B, N).contiguous()
    exact = ops.exact_gather_dist_f16(metric, qd, xd, rows).cpu().numpy()  # the arithmetic of the search's exact stage
    assert np.array_equal(exact.view(np.uint32), ops.exact_gather_dist(metric, qd, ops.to_dev(x), rows).cpu().numpy().view(np.uint32))
    bound = np.sort(np.where(ok[None, :], exact, np.inf), axis=1)[:, k - 1].astype(F)
    cand, count, qn, qf, scores = ops.flat_filter_f16(metric, qd, xd, norms, ops.to_dev(bound), valid_bits=bits, scores=True)
    torch.cuda.synchronize()
    cand, count, qn, qf, scores, norms = (t.cpu().numpy() for t in (cand, count, qn, qf, scores, norms))
    c_rel, c_abs = ops.flat_f16_slack(metric, D)
    q64 = q.astype(np.float64)
    assert (qf >= 2.0 ** -13 * np.abs(q64).sum(1)).all() and (qf <= 1.01 * 2.0 ** -13 * np.abs(q64).sum(1)).all()
    slack32 = ((F(c_rel) * (norms[None, :N] + qn[:, None]).astype(F) + F(c_abs)).astype(F) + qf[:, None]).astype(F)  # as the kernel adds it
    slack = slack32.astype(np.float64)
    x64 = x.astype(np.float64)
    d64 = ((x64[None] - q64[:, None]) ** 2).sum(-1) if metric == 1 else 1.0 - q64 @ x64.T
    assert np.isfinite(scores).all() and scores.shape == (B, N)
    worst = 0.0
    for b in range(B):
        assert 0 < count[b] <= ops.flat_list_capacity()
        lst = cand[b, :count[b]]
        assert len(set(lst.tolist())) == len(lst), 'a row listed twice'
        assert ((lst >= 0) & (lst < N)).all() and ok[lst].all(), 'an invalid row listed'
        need = np.nonzero(ok & (exact[b] <= bound[b]))[0]
        assert len(need) >= k and np.isin(need, lst).all(), (family, b, 'a row within the bound is missing')
        assert (d64[b, lst] <= float(bound[b]) + 2 * slack[b, lst]).all(), 'a listed row lies beyond the bound by more than twice the slack'
        # ... and the kernel's comparison, redone on its own scores, is the list
        passed = np.nonzero(ok & ~(scores[b] > (bound[b] + slack32[b]).astype(F)))[0]
        assert np.array_equal(np.sort(lst), passed)
        worst = max(worst, float((np.abs(scores[b].astype(np.float64) - d64[b]) / slack[b])[ok].max()))
    print(f'f16 filter |v - d| / slack: family={family!r} D={D} metric={metric} worst={worst:.4f}')
    assert worst <= 1.0  # (DESIGN.md section 3.6 records the measured values; above 1 the derivation's assumptions are refuted)


# ---- non-finite inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', [1, 2, 3])
def test_non_finite_inputs_answer_as_the_f32_index_over_the_widened_rows(ops, metric):
    rs = np.random.RandomState(9)
    x, q = rs.randn(5000, 16).astype(F), rs.randn(8, 16).astype(F)
    q[1, 3], q[2, 0], q[3, 15], q[4, :], q[5, :], q[6, :] = np.nan, np.inf, -np.inf, np.nan, 0.0, 1e30 * q[6]
    x[77, 5], x[4999, 0], x[12, :] = 1e6, -7e4, 0.0  # (beyond the f16 range: stored as +inf / -inf; COSINE normalises them first)
    new, ref, qr = _pair(metric, 16, x, q)
    stored = new._vectors[:5000].cpu().numpy()
    assert (np.isinf(stored).sum() == 2) == (metric != 3) and stored.dtype == H
    for k in (1, 10, 64, 100):
        want, got = ref.search_batch(qr, limit=k), new.search_batch(q, limit=k)
        _same(got, want, (metric, k))
        assert new.last_overflowed == ref.last_overflowed
        assert k > 64 or (new.last_flat_filter == 'f16x2' and new.last_overflowed >= 4)  # (limit 100, 5000 rows: no filter runs)


# ---- lifecycle ------------------------------------------------------------------------------------------------------------------------
def test_updated_rows_are_rounded_again_and_carry_their_norms(ops):
    rs = np.random.RandomState(4)
    x = rs.randn(6000, 33).astype(F)
    new, ref = _index(1, 33, x, dtype=np.float16), _index(1, 33, f16(x))
    ids = rs.choice(6000, 100, replace=False)
    moved = (40.0 + rs.randn(100, 33)).astype(F)  # far from where the rows were: a stale norm would put the filter's score off by ~10^4
    new.update_with_ids(moved, ids)
    ref.update_with_ids(f16(moved), ids)
    assert np.array_equal(new._vectors[ids].cpu().numpy(), moved.astype(H))
    assert np.array_equal(new._norms[:6000].cpu().numpy().view(np.uint32), ref._norms[:6000].cpu().numpy().view(np.uint32))
    q = np.concatenate([f16(moved[:20]), rs.randn(5, 33).astype(F)])
    got = new.search_batch(q, limit=10)
    _same(got, ref.search_batch(q, limit=10), 'after update_with_ids')
    assert np.array_equal(got[1][:20, 0], ids[:20]) and (got[0][:20, 0] == 0.0).all() and new.last_overflowed == 0


def test_dump_and_load_across_the_dtypes(ops, tmp_path):
    import torch
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.enums import Metric

    rs = np.random.RandomState(6)
    x, q = rs.randn(5000, 32).astype(F), rs.randn(7, 32).astype(F)
    half, full, ref = _index(1, 32, x, dtype=np.float16), _index(1, 32, x), _index(1, 32, f16(x))
    for idx in (half, full, ref):
        idx.delete([5, 4000])
    want, want_full = ref.search_batch(q, limit=10), full.search_batch(q, limit=10)
    half.dump(tmp_path / 'f16.bin'), full.dump(tmp_path / 'f32.bin')
    for name, dt in (('f16.bin', H), ('f32.bin', F)):
        state = np.load(tmp_path / name, allow_pickle=True)[0]
        assert state['format'] == FlatGpuIndex.FORMAT and state['vectors'].dtype == dt  # (one format; the array in the index's dtype)
    for file, dtype, expect in (('f16.bin', np.float16, want), ('f32.bin', np.float16, want),  # (f32 into an f16 index rounds)
                                ('f16.bin', np.float32, want), ('f32.bin', np.float32, want_full)):  # (f16 into an f32 index widens)
        back = FlatGpuIndex(32, dtype=dtype, metric=Metric.EUCLIDEAN, index_file=tmp_path / file)
        assert back._vectors.dtype == (torch.float16 if dtype == np.float16 else torch.float32) and back.size == 4998
        _same(back.search_batch(q, limit=10), expect, (file, dtype))
        assert back.last_flat_filter == ('f16x2' if dtype == np.float16 else 'f32') and back.last_overflowed == 0
        _same(back.search_batch(q, limit=70), (ref if expect is want else full).search_batch(q, limit=70), (file, dtype, 'limit 70'))
        assert np.array_equal(back._norms[:5000].cpu().numpy(), (ref if expect is want else full)._norms[:5000].cpu().numpy())


def test_growth_past_the_initial_size_and_reset(ops):
    import torch

    rs = np.random.RandomState(7)
    x, q = rs.randn(5000, 24).astype(F), rs.randn(9, 24).astype(F)
    new = _index(2, 24, x[:700], dtype=np.float16, initial_size=1000, expand_step_size=1000)
    for lo in range(700, 5000, 900):
        new.add_with_ids(x[lo:lo + 900], np.arange(lo, min(lo + 900, 5000)))
    assert new.capacity == 5000 and new.size == 5000 and new._vectors.dtype == torch.float16 and new._vectors.shape == (5000, 24)
    _same(new.search_batch(q, limit=10), _index(2, 24, f16(x)).search_batch(q, limit=10), 'grown')
    new.reset()
    assert new.size == 0 and new._vectors is None
    new.add_with_ids(x[:10], np.arange(10))
    assert new._vectors.dtype == torch.float16
