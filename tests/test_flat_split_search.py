"""The split-bf16 filter of the exact float32 search on the GPU ("split filter"): ``flat_filter='bf16x3'``
returns the default index's answer bit for bit; at the stage level every row within the bound is listed; offset data no longer
overflows; non-finite inputs keep the convention."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

F = np.float32


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _index(metric, D, x, cls=None, **kw):
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.enums import Metric

    idx = (cls or FlatGpuIndex)(D, metric=Metric(metric), initial_size=max(len(x), 1), **kw)
    idx.add_with_ids(x, np.arange(len(x)))
    return idx


def _same(got, want, what):
    (gd, gi), (wd, wi) = got, want
    assert gi.dtype == np.int64 and gd.dtype == np.float32
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:5], gi[gi != wi][:5], wi[gi != wi][:5])
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (what, 'distance bits')


# ---- the same answer, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [4097, 4225, 20000])  # the filter engages above 4096 rows; a tile is 128 rows: 1 row, 1 tile + 1, many
@pytest.mark.parametrize('D', [1, 5, 16, 33, 128, 770])
def test_split_filter_gives_the_default_index_its_bits(ops, D, N):
    rs = np.random.RandomState(1000 * D + N % 997)
    x = rs.randn(N, D).astype(F)
    x[100:140] = x[100]  # a block of identical rows: ties ordered by id
    q = rs.randn(129, D).astype(F)
    q[0] = x[100]        # a query equal to stored rows
    gone = np.arange(0, N, 3)
    keep = np.arange(1, N, 5)
    for metric in (1, 2, 3):
        ref, new = _index(metric, D, x), _index(metric, D, x, flat_filter='bf16x3')
        assert (new.centre_ is not None) == (metric == 1) and ref.centre_ is None
        for B in (1, 129):
            for k in (1, 10, 64):
                got, want = new.search_batch(q[:B], limit=k), ref.search_batch(q[:B], limit=k)
                _same(got, want, (metric, B, k))
                assert new.last_flat_filter == 'bf16x3' and ref.last_flat_filter == 'f32'
                if metric == 1:
                    assert got[0][0, 0] == 0.0 and got[1][0, 0] == 100 and (k < 10 or list(got[1][0, :10]) == list(range(100, 110)))
        _same(new.search_batch(q, limit=10, indices=keep), ref.search_batch(q, limit=10, indices=keep), (metric, 'a fifth kept'))
        assert new.last_flat_filter == 'bf16x3'
        for idx in (ref, new):
            idx.delete(gone)
        for B, k in ((129, 10), (1, 64)):
            _same(new.search_batch(q[:B], limit=k), ref.search_batch(q[:B], limit=k), (metric, B, k, 'a third deleted'))
            assert new.last_flat_filter == 'bf16x3'


def test_small_tables_and_limits_beyond_64_run_no_split_filter(ops):
    rs = np.random.RandomState(2)
    x, q = rs.randn(9000, 16).astype(F), rs.randn(3, 16).astype(F)
    ref, new = _index(1, 16, x), _index(1, 16, x, flat_filter='bf16x3')
    _same(new.search_batch(q, limit=100), ref.search_batch(q, limit=100), 'limit 100')
    assert new.last_flat_filter == 'f32'  # (the k > 64 path keeps the f32 filter)
    _same(new.search_batch(q, limit=10), ref.search_batch(q, limit=10), 'limit 10')
    assert new.last_flat_filter == 'bf16x3'
    small = _index(1, 16, x[:4096], flat_filter='bf16x3')
    _same(small.search_batch(q, limit=10), _index(1, 16, x[:4096]).search_batch(q, limit=10), '4096 rows')
    assert small.last_flat_filter is None and small.last_overflowed == 0


def test_graph_index_exact_fallback_uses_the_split_filter(ops):
    from annlite_amd.core.index.hnsw_flat_gpu import HnswFlatGpuIndex

    rs = np.random.RandomState(3)
    x, q = (50.0 + rs.randn(4225, 16)).astype(F), (50.0 + rs.randn(9, 16)).astype(F)
    g = _index(1, 16, x, cls=HnswFlatGpuIndex, flat_filter='bf16x3')
    want = _index(1, 16, x).search_batch(q, limit=10)
    _same(g.search_exhaustive(q, limit=10), want, 'search_exhaustive')
    assert g.last_flat_filter == 'bf16x3' and g.centre_ is not None
    _same(g.search_batch(q, limit=10, indices=np.arange(0, 4225, 2)), _index(1, 16, x).search_batch(q, limit=10, indices=np.arange(0, 4225, 2)),
          'filtered, answered exactly')
    assert g.last_flat_filter == 'bf16x3'
    g.search_batch(q, limit=10)
    assert g.last_flat_filter is None  # (a walk)


def test_updated_rows_carry_their_centred_norms(ops):
    rs = np.random.RandomState(4)
    x = rs.randn(6000, 33).astype(F)
    ref, new = _index(1, 33, x), _index(1, 33, x, flat_filter='bf16x3')
    centre = new.centre_.copy()
    ids = rs.choice(6000, 100, replace=False)
    moved = (40.0 + rs.randn(100, 33)).astype(F)  # far from where the rows were: a stale norm would put the filter's score off by ~10^4
    for idx in (ref, new):
        idx.update_with_ids(moved, ids)
    assert np.array_equal(new.centre_, centre)  # (frozen since the first batch)
    q = np.concatenate([moved[:20], rs.randn(5, 33).astype(F)])
    got = new.search_batch(q, limit=10)
    _same(got, ref.search_batch(q, limit=10), 'after update_with_ids')
    assert np.array_equal(got[1][:20, 0], ids[:20]) and (got[0][:20, 0] == 0.0).all() and new.last_overflowed == 0


def test_dump_and_load_carry_the_centre(ops, tmp_path):
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.enums import Metric

    rs = np.random.RandomState(6)
    x, q = (1000.0 + rs.randn(5000, 32)).astype(F), (1000.0 + rs.randn(7, 32)).astype(F)
    ref, new = _index(1, 32, x[:4500]), _index(1, 32, x[:4500], flat_filter='bf16x3')
    for idx in (ref, new):
        idx.add_with_ids(x[4500:], np.arange(4500, 5000))
    assert np.array_equal(new.centre_, x[:4500].mean(axis=0, dtype=F)) or np.allclose(new.centre_, x[:4500].mean(axis=0), rtol=1e-5)
    want = ref.search_batch(q, limit=10)
    new.dump(tmp_path / 'split.bin'), ref.dump(tmp_path / 'f32.bin')
    back = FlatGpuIndex(32, metric=Metric.EUCLIDEAN, flat_filter='bf16x3', index_file=tmp_path / 'split.bin')
    assert np.array_equal(back.centre_, new.centre_)  # (the first batch's mean, not the mean of all rows)
    _same(back.search_batch(q, limit=10), want, 'loaded with its centre')
    assert back.last_flat_filter == 'bf16x3' and back.last_overflowed == 0
    old = FlatGpuIndex(32, metric=Metric.EUCLIDEAN, flat_filter='bf16x3', index_file=tmp_path / 'f32.bin')  # a file without the key
    assert np.allclose(old.centre_, x.mean(axis=0), rtol=1e-5)
    _same(old.search_batch(q, limit=10), want, 'loaded without a centre')
    assert old.last_overflowed == 0
    plain = FlatGpuIndex(32, metric=Metric.EUCLIDEAN, index_file=tmp_path / 'split.bin')  # ... and the key does not trouble an f32 index
    _same(plain.search_batch(q, limit=10), want, 'f32 index, file with a centre')
    assert plain.centre_ is None
    new.reset()
    assert new.centre_ is None


# ---- the stage alone: a superset, and the measured error ------------------------------------------------------------------------------
def _family(name, N, D, B, rs):
    if name == 'offset':
        return (1000.0 + 0.01 * rs.randn(N, D)).astype(F), (1000.0 + 0.01 * rs.randn(B, D)).astype(F)
    if name == 'near-duplicates':
        x = rs.randn(N, D).astype(F)
        return x, (x[:B] * F(1 + 2 ** -20) + F(1e-6) * rs.randn(B, D)).astype(F)
    if name == 'identical':
        x = rs.randn(N, D).astype(F)
        return x, x[7:7 + B].copy()
    if name == 'mixed magnitudes':
        scale = (10.0 ** rs.uniform(-6, 6, size=(1, D))).astype(F)
        return (rs.randn(N, D) * scale).astype(F), (rs.randn(B, D) * scale[:, ::-1]).astype(F)
    if name == 'tiny':
        return (1e-18 * rs.randn(N, D)).astype(F), (1e-18 * rs.randn(B, D)).astype(F)
    assert name == 'adversarial mantissas'
    m = F(1 + 2.0 ** -8 - 2.0 ** -20)
    mk = lambda n: (m * rs.choice([-1.0, 1.0], size=(n, D)) * 2.0 ** rs.randint(-3, 4, size=(n, D))).astype(F)
    return mk(N), mk(B)


FAMILIES = ['offset', 'near-duplicates', 'identical', 'mixed magnitudes', 'tiny', 'adversarial mantissas']
CASES = [(1, True), (1, False), (2, False)]  # (metric, with a centre): a centre is EUCLIDEAN's


@pytest.mark.parametrize('metric,centred', CASES)
@pytest.mark.parametrize('D', [5, 128])
@pytest.mark.parametrize('family', FAMILIES)
def test_stage_lists_every_row_within_the_bound(ops, family, D, metric, centred):
    import torch
    from annlite_amd.core.index.row_store import RowStoreIndex

    N, B, k = 4225, 8, 10
    rs = np.random.RandomState(17 * D + len(family))
    x, q = _family(family, N, D, B, rs)
    xd, qd = ops.to_dev(x), ops.to_dev(q)
    flags = torch.ones(((N + 31) // 32 + 2) * 32, dtype=torch.bool, device=xd.device)
    flags[N:] = False
    flags[torch.arange(3, N, 7, device=xd.device)] = False  # (under `cap` valid rows: no list can overflow)
    bits = RowStoreIndex._pack_bits(flags)
    ok = flags[:N].cpu().numpy()
    mu = ops.to_dev(x.mean(axis=0, dtype=np.float64).astype(F)) if centred else None
    norms = ops.flat_centred_norms(xd, mu) if centred else ops.flat_row_norms(xd)
    rows = torch.arange(N, dtype=torch.int64, device=xd.device)[None, :].expand(B, N).contiguous()
    exact = ops.exact_gather_dist(metric, qd, xd, rows).cpu().numpy()  # the arithmetic of the search's exact stage
    bound = np.sort(np.where(ok[None, :], exact, np.inf), axis=1)[:, k - 1].astype(F)
    cand, count, qn, scores = ops.flat_filter_split(metric, qd, xd, norms, ops.to_dev(bound), centre=mu, valid_bits=bits, scores=True)
    torch.cuda.synchronize()
    cand, count, qn, scores, norms = (t.cpu().numpy() for t in (cand, count, qn, scores, norms))
    c_rel, c_abs = ops.flat_split_slack(metric, D)
    slack = (F(c_rel) * (norms[None, :N] + qn[:, None]).astype(F) + F(c_abs)).astype(np.float64)
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
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
        passed = np.nonzero(ok & ~(scores[b] > (bound[b] + (F(c_rel) * (norms[:N] + qn[b]).astype(F) + F(c_abs))).astype(F)))[0]
        assert np.array_equal(np.sort(lst), passed)
        worst = max(worst, float((np.abs(scores[b].astype(np.float64) - d64[b]) / slack[b])[ok].max()))
    print(f'split filter |v - d| / slack: family={family!r} D={D} metric={metric} centred={centred} worst={worst:.4f}')
    assert worst <= 1.0  # (DESIGN.md section 3.6 records the measured values)


# ---- offset data ----------------------------------------------------------------------------------------------------------------------
def test_offset_data_overflows_the_f32_filter_and_not_the_centred_split_filter(ops):
    rs = np.random.RandomState(8)
    x, q = (1000.0 + rs.randn(8192, 32)).astype(F), (1000.0 + rs.randn(16, 32)).astype(F)
    ref, new = _index(1, 32, x), _index(1, 32, x, flat_filter='bf16x3', centre='mean')
    want, got = ref.search_batch(q, limit=10), new.search_batch(q, limit=10)
    assert ref.last_overflowed == 16 and new.last_overflowed == 0
    _same(got, want, 'offset data')
    uncentred = _index(1, 32, x, flat_filter='bf16x3', centre=None)  # (the split filter alone does not help: the centre does)
    _same(uncentred.search_batch(q, limit=10), want, 'offset data, no centre')
    assert uncentred.last_overflowed == 16 and uncentred.centre_ is None


# ---- non-finite inputs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', [1, 2])
def test_non_finite_inputs_answer_as_the_default_index(ops, metric):
    rs = np.random.RandomState(9)
    x, q = rs.randn(5000, 16).astype(F), rs.randn(6, 16).astype(F)
    q[1, 3], q[2, 0], q[3, 15], q[4, :] = np.nan, np.inf, -np.inf, np.nan
    ref, new = _index(metric, 16, x), _index(metric, 16, x, flat_filter='bf16x3')
    bad = x[[77, 4999]].copy()
    bad[0, 5], bad[1, 0] = np.inf, -np.inf
    for idx in (ref, new):
        idx.update_with_ids(bad, [77, 4999])  # (after the first batch: the centre is that batch's finite mean)
    for k in (1, 10, 64):
        want, got = ref.search_batch(q, limit=k), new.search_batch(q, limit=k)
        _same(got, want, (metric, k))
        assert new.last_overflowed == ref.last_overflowed >= 4 and new.last_flat_filter == 'bf16x3'
