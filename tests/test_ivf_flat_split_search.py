"""The split-bf16 filter over cell tiles on the GPU (``IvfFlatGpuIndex(cell_filter='bf16x3')``, ``annlite_ivf_flat_search_topk_split``;
DESIGN.md section 3.7, "split filter over cell tiles"): the default cell index's answer bit for bit; at the stage level every probed
row within the bound is listed and the score stays inside the slack; offset data no longer overflows; mutations, non-finite inputs
and ``dump`` / ``load`` keep the bits.

The data and the yardstick are ``test_ivf_flat_search``'s (a hand-set codebook: corners of a cube)."""
import numpy as np
import pytest

from conftest import has_gpu
from test_flat_split_search import FAMILIES, _family
from test_ivf_flat_search import SIZES, _centroids, _index, _probed, _queries, _rows, _same, _vq, _yardstick

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

F = np.float32


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _pair(metric, D, vq, x, **kw):
    """(the default index, the split-filter index) over the same rows and codebook"""
    return _index(metric, D, vq, x, **kw), _index(metric, D, vq, x, cell_filter='bf16x3', **kw)


# ---- 1. the same answer, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', [1, 2, 3])
@pytest.mark.parametrize('D', [5, 96, 128])  # the scalar staging path with Dp = 16; a whole last stage with Dp = D; the headline
def test_split_cell_filter_gives_the_default_index_its_bits(ops, metric, D):
    C = len(SIZES)
    rs = np.random.RandomState(100 * D + metric)
    x, cell = _rows(rs, SIZES, D)
    dup = np.flatnonzero(cell == 4)[:12]
    x[dup] = x[dup[0]]  # ties inside a probed cell: the lower id first
    ref, new = _pair(metric, D, _vq(C, D, metric), x)
    assert (new.cell_centres_ is not None) == (metric == 1) and ref.cell_centres_ is None
    assert (new._cell_cnorms is not None) == (metric == 1) and ref._cell_cnorms is None
    qs = {B: _queries(rs, C, D, B) for B in (1, 5, 300)}
    qs[5][2] = x[dup[3]]                          # a query equal to a stored (and duplicated) row
    qs[300][7] = x[np.flatnonzero(cell == 1)[0]]  # ... and to the only row of its cell
    for P in (1, 3, C - 1):
        assert ops.ivf_flat_stages(sum(sorted(SIZES)[-P:]))  # (not the exact-only route)
        for B, q in qs.items():
            probed = _probed(new, q, P)
            for k in (1, 10, 64):
                got = new.search_batch(q, limit=k, n_probe=P)
                assert new.last_cell_filter == 'bf16x3'
                _same(got, ref.search_batch(q, limit=k, n_probe=P), (P, B, k, 'default index'))
                assert ref.last_cell_filter == 'f32'
                _same(got, _yardstick(ops, new, q, k, P, probed=probed), (P, B, k, 'yardstick'))
            assert new.last_overflowed == 0
        if metric == 1:
            got = new.search_batch(qs[5], limit=12, n_probe=P)
            assert got[0][2, 0] == 0.0 and np.array_equal(got[1][2], np.sort(dup))  # self-match at exactly 0, its duplicates by id
            got = new.search_batch(qs[300], limit=1, n_probe=P)
            assert got[0][7, 0] == 0.0 and cell[got[1][7, 0]] == 1


def test_routes_that_run_no_cell_filter(ops):
    rs = np.random.RandomState(2)
    D, sizes = 32, [3000, 2500, 1000]
    x, _ = _rows(rs, sizes, D)
    ref, new = _pair(1, D, _vq(3, D, 1), x, n_probe=2)
    q = _queries(rs, 3, D, 9)
    _same(new.search_batch(q, limit=10), ref.search_batch(q, limit=10), 'two cells')
    assert new.last_cell_filter == 'bf16x3' and ref.last_cell_filter == 'f32'
    _same(new.search_batch(q, limit=10, n_probe=1), ref.search_batch(q, limit=10, n_probe=1), 'exact-only')
    assert new.last_cell_filter is None and ref.last_cell_filter is None  # (at most 3000 probed rows: no filter)
    _same(new.search_batch(q, limit=100), ref.search_batch(q, limit=100), 'limit 100')
    assert new.last_cell_filter is None
    _same(new.search_batch(q, limit=10, n_probe=3), ref.search_batch(q, limit=10, n_probe=3), 'every cell')
    assert new.last_cell_filter is None and new.last_flat_filter == 'f32'
    new.reset()
    assert new.cell_centres_ is None
    d, i = new.search_batch(q, limit=10)
    assert (i == -1).all() and new.last_cell_filter is None


# ---- 2. query tiles and stages -------------------------------------------------------------------------------------------------------
def test_two_query_tiles_in_one_cell(ops):
    rs = np.random.RandomState(3)
    D, C = 32, 2
    x, cell = _rows(rs, [5000, 4500], D)
    ref, new = _pair(1, D, _vq(C, D, 1), x, n_probe=1)
    q = _queries(rs, C, D, 300)
    q[:200] = (_centroids(C, D)[0] + 0.5 * rs.randn(200, D)).astype(np.float32)  # 200 queries probe cell 0: two tiles of 128 slots
    probed = _probed(new, q, 1)
    assert int((probed[2][:, 0] == 0).sum().item()) > 128
    for k in (10, 64):
        got = new.search_batch(q, limit=k)
        _same(got, ref.search_batch(q, limit=k), k)
        _same(got, _yardstick(ops, new, q, k, 1, probed=probed), k)
        assert new.last_overflowed == 0 and new.last_cell_filter == 'bf16x3'


def test_several_filter_stages_and_no_overflow(ops):
    rs = np.random.RandomState(5)
    N, D, C, P, B = 300_000, 16, 4, 2, 64
    x = rs.randn(N, D).astype(np.float32)
    q = rs.randn(B, D).astype(np.float32)
    vq = _vq(C, D, 1)
    vq._codebook = np.zeros((C, D), np.float32)
    vq._codebook[:, 0] = [1, 1, -1, -1]  # the quadrants of the first two coordinates: four cells of about N / 4 rows
    vq._codebook[:, 1] = [1, -1, 1, -1]
    new = _index(1, D, vq, x, n_probe=P, cell_filter='bf16x3')
    new._seal()
    strides = ops.ivf_flat_stages(int(new._sizes_cum[P - 1]))
    assert int(new._sizes_cum[P - 1]) > 32 * 4096 and len(strides) >= 3, strides  # the first sample + at least two filter stages
    got10 = new.search_batch(q, limit=10)
    assert new.last_overflowed == 0 and new.last_cell_filter == 'bf16x3'
    got64 = new.search_batch(q, limit=64)
    assert new.last_overflowed == 0
    sub = np.arange(0, B, 4)  # 16 of the queries
    probed = _probed(new, q[sub], P)
    _same((got10[0][sub], got10[1][sub]), _yardstick(ops, new, q[sub], 10, P, probed=probed), 'k=10')
    _same((got64[0][sub], got64[1][sub]), _yardstick(ops, new, q[sub], 64, P, probed=probed), 'k=64')


# ---- 3. offset data ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def offset():
    """(x, q, codebook): D = 32, two cells of 5000 / 4500 rows around 1000 + the cube's corners (noise 0.3), 50 queries (noise 0.5)"""
    rs = np.random.RandomState(7)
    D = 32
    codebook = (F(1000.0) + _centroids(2, D)).astype(F)
    x, _ = _rows(rs, [5000, 4500], D)
    return (x + F(1000.0)).astype(F), (_queries(rs, 2, D, 50) + F(1000.0)).astype(F), codebook


def _offset_vq(codebook):
    vq = _vq(2, codebook.shape[1], 1)
    vq._codebook = codebook.copy()
    return vq


def test_offset_data_overflows_the_f32_cell_filter_and_not_the_split_one(ops, offset):
    x, q, codebook = offset
    ref, new = _pair(1, 32, _offset_vq(codebook), x, n_probe=1)
    want, got = ref.search_batch(q, limit=10), new.search_batch(q, limit=10)
    assert ref.last_overflowed == 50  # every row of the probed cell passes the f32 comparison: 4500 / 5000 > 4096
    assert new.last_overflowed == 0 and new.last_cell_filter == 'bf16x3'
    _same(got, want, 'offset data')
    assert np.array_equal(new.cell_centres_, codebook)
    counts = ops.flat_list_counts(new._ws, len(q)).cpu().numpy()
    print(f'offset layout: split filter lists mean={counts.mean():.1f} max={counts.max()}')
    assert counts.max() <= 64  # (test_ivf_flat_split_host restates the comparison in numpy: a few dozen rows)


# ---- 4. the stage alone: a superset, and the measured error --------------------------------------------------------------------------
CASES = [(1, True), (1, False), (2, False)]  # (metric, with centres): a centre is EUCLIDEAN's


@pytest.mark.parametrize('metric,centred', CASES)
@pytest.mark.parametrize('D', [5, 128])
@pytest.mark.parametrize('family', FAMILIES)
def test_stage_lists_every_probed_row_within_the_bound(ops, family, D, metric, centred):
    import torch
    from annlite_amd.core.index.row_store import RowStoreIndex

    sizes, B, P, k = [2000, 2000, 225], 8, 2, 10
    N, C = sum(sizes), len(sizes)
    rs = np.random.RandomState(17 * D + len(family))
    x, q = _family(family, N, D, B, rs)
    cent = _centroids(C, D)
    cell = rs.permutation(np.repeat(np.arange(C), sizes))
    cells = np.stack([np.arange(B) % C, (np.arange(B) + 1) % C], axis=1).astype(np.int32)  # every pair of cells, either order
    x, q = (x + cent[cell]).astype(F), (q + cent[cells[:, 0]]).astype(F)
    xd, qd = ops.to_dev(x), ops.to_dev(q)
    dev = xd.device
    flags = torch.ones(((N + 31) // 32 + 2) * 32, dtype=torch.bool, device=dev)
    flags[N:] = False
    flags[torch.arange(3, N, 7, device=dev)] = False  # (under `cap` valid rows: no list can overflow)
    bits = RowStoreIndex._pack_bits(flags)
    ok = flags[:N].cpu().numpy()
    # the sealed view, over ALL rows: the dead ones are the bitmap's to drop
    perm = np.argsort(cell, kind='stable').astype(np.int32)
    end = np.cumsum(sizes)
    cell_rows = np.stack([end - sizes, end], axis=1).astype(np.int64)
    cell_order = np.argsort(-np.asarray(sizes), kind='stable').astype(np.int32)
    cell_of = ops.to_dev(cell.astype(np.int32))
    centres = ops.to_dev(np.stack([x[cell == c].mean(axis=0, dtype=np.float64) for c in range(C)]).astype(F)) if centred else None
    norms = ops.ivf_flat_centred_norms(xd, centres, cell_of) if centred else ops.flat_row_norms(xd)
    probed = (cell[None, :, None] == cells[:, None, :])        # [B, N, P]
    live = probed.any(axis=2) & ok[None, :]
    rows = torch.arange(N, dtype=torch.int64, device=dev)[None, :].expand(B, N).contiguous()
    exact = ops.exact_gather_dist(metric, qd, xd, rows).cpu().numpy()  # the arithmetic of the search's exact stage
    bound = np.sort(np.where(live, exact, np.inf), axis=1)[:, k - 1].astype(F)
    cand, count, pn, scores = ops.ivf_flat_filter_split(metric, qd, xd, norms, ops.to_dev(bound), ops.to_dev(cells), C, ops.to_dev(perm),
                                                        ops.to_dev(cell_rows), ops.to_dev(cell_order), max(sizes), centres=centres,
                                                        cell_of=cell_of if centred else None, valid_bits=bits, scores=True)
    torch.cuda.synchronize()
    cand, count, pn, scores, norms = (t.cpu().numpy() for t in (cand, count, pn, scores, norms))
    c_rel, c_abs = ops.flat_split_slack(metric, D)
    qn = np.where(probed, pn[:, None, :], 0).sum(axis=2).astype(F)  # [B, N]: the norm of the pair whose cell holds the row
    a = (norms[None, :N] + qn).astype(F)
    slack32 = (F(c_rel) * a + F(c_abs)).astype(F)
    slack = slack32.astype(np.float64)
    x64, q64 = x.astype(np.float64), q.astype(np.float64)
    d64 = ((x64[None] - q64[:, None]) ** 2).sum(-1) if metric == 1 else 1.0 - q64 @ x64.T
    assert scores.shape == (B, N) and np.isfinite(scores[live]).all() and np.isnan(scores[~live]).all()  # (not evaluated: the caller's NaN)
    worst = 0.0
    for b in range(B):
        assert 0 < count[b] <= ops.flat_list_capacity()
        lst = cand[b, :count[b]]
        assert len(set(lst.tolist())) == len(lst), 'a row listed twice'
        assert ((lst >= 0) & (lst < N)).all() and live[b, lst].all(), 'a row listed that is not a live probed row'
        need = np.nonzero(live[b] & (exact[b] <= bound[b]))[0]
        assert len(need) >= k and np.isin(need, lst).all(), (family, b, 'a row within the bound is missing')
        assert (d64[b, lst] <= float(bound[b]) + 2 * slack[b, lst]).all(), 'a listed row lies beyond the bound by more than twice the slack'
        # ... and the kernel's comparison, redone on its own scores and pair norms, is the list
        passed = np.nonzero(live[b] & ~(scores[b] > (bound[b] + slack32[b]).astype(F)))[0]
        assert np.array_equal(np.sort(lst), passed)
        worst = max(worst, float((np.abs(scores[b].astype(np.float64) - d64[b]) / slack[b])[live[b]].max()))
    print(f'split cell filter |v - d| / slack: family={family!r} D={D} metric={metric} centred={centred} worst={worst:.4f}')
    assert worst <= 1.0  # (the proof's condition; DESIGN.md section 3.7 records the measured values)


# ---- 5. mutations ------------------------------------------------------------------------------------------------------------------------
def test_deletes_indices_updates_and_later_adds(ops):
    rs = np.random.RandomState(13)
    D, sizes = 32, [4500, 3000, 2000, 400, 100]
    C, P = len(sizes), 2
    x, cell = _rows(rs, sizes, D)
    N = len(x)
    ref, new = _pair(1, D, _vq(C, D, 1), x, n_probe=P, expand_step_size=1024)
    q = _queries(rs, C, D, 150)

    def both(what, **kw):
        got = new.search_batch(q, **kw)
        _same(got, ref.search_batch(q, **kw), what)
        assert new.last_cell_filter == 'bf16x3' and new.last_overflowed == 0
        return got

    def column(what):
        n = new._n_rows
        want = ops.ivf_flat_centred_norms(new._vectors, new._cell_centres_dev, new._cell_of, n=n)
        assert np.array_equal(new._cell_cnorms[:n].cpu().numpy().view(np.uint32), want[:n].cpu().numpy().view(np.uint32)), what

    column('first batch')
    # a third of the rows, among them EVERY row of cell 1 (which queries probe)
    dead = np.union1d(np.flatnonzero(cell == 1), rs.choice(N, size=N // 3 - sizes[1], replace=False))
    for idx in (ref, new):
        idx.delete(dead.tolist())
    for k in (10, 64):
        assert not np.isin(both(('deleted', k), limit=k)[1], dead).any()
    keep = rs.choice(N, size=N // 5, replace=False)
    got = new.search_batch(q, limit=16, indices=keep)
    _same(got, ref.search_batch(q, limit=16, indices=keep), 'indices')
    assert np.isin(got[1][got[1] >= 0], np.setdiff1d(keep, dead)).all()
    # update_with_ids with a vector of ANOTHER cell: the row moves, and its norm is the one against its new centroid
    a = int(np.setdiff1d(np.flatnonzero(cell == 0), dead)[0])
    moved = (_centroids(C, D)[3] + 0.01 * rs.randn(D)).astype(np.float32)
    before = float(new._cell_cnorms[a].item())
    for idx in (ref, new):
        idx.update_with_ids(moved[None, :], [a])
    assert int(new._cell_of[a].item()) == 3
    after = float(new._cell_cnorms[a].item())
    assert after != before and after < 0.01 * D  # (|moved - centroid 3|^2 ~ 1e-4 D; against centroid 0 it would be 36)
    column('updated')
    both('updated', limit=10)
    d, i = new.search_batch(moved[None, :], limit=1, n_probe=1)
    assert i[0, 0] == a and d[0, 0] == 0.0
    # a later add (the store grows, the seal is rebuilt): rows into cell 1 again, under new ids
    more = (_centroids(C, D)[1] + 0.3 * rs.randn(700, D)).astype(np.float32)
    centres = new.cell_centres_.copy()
    for idx in (ref, new):
        idx.add_with_ids(more, np.arange(N, N + 700))
    assert new.capacity >= N + 700 and np.array_equal(new.cell_centres_, centres)
    column('added')
    assert (both('added', limit=10)[1] >= N).any()


# ---- 6. non-finite inputs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', [1, 2])
def test_non_finite_queries(ops, metric):
    rs = np.random.RandomState(19)
    D, sizes = 32, [4500, 3000, 2000, 40]
    x, _ = _rows(rs, sizes, D)
    ref, new = _pair(metric, D, _vq(len(sizes), D, metric), x, n_probe=2)
    q = _queries(rs, len(sizes), D, 9)
    q[1, 3] = np.inf
    q[2, 0] = -np.inf
    q[4, :] = np.nan
    q[6, 10] = np.nan
    for k in (10, 64):
        _same(new.search_batch(q, limit=k), ref.search_batch(q, limit=k), k)
        assert new.last_cell_filter == 'bf16x3' and new.last_overflowed == ref.last_overflowed


def test_a_nan_centroid_takes_the_overflow_route(ops):
    rs = np.random.RandomState(21)
    D, sizes = 32, [4500, 3000, 2000, 40]
    C = len(sizes)
    x, cell = _rows(rs, sizes, D)
    q = _queries(rs, C, D, 40)
    # a codebook with a NaN in one centroid, end to end: whatever the selection makes of that cell, both indexes agree
    vq = _vq(C, D, 1)
    vq._codebook[1, 2] = np.nan
    ref, new = _pair(1, D, vq, x, n_probe=2)
    assert np.isnan(new.cell_centres_[1, 2])
    _same(new.search_batch(q, limit=10), ref.search_batch(q, limit=10), 'NaN in the codebook')
    # ... and a NaN in the snapshot of a cell that holds 4500 rows: its scores are NaN, its rows pass, the lists overflow
    ref, new = _pair(1, D, _vq(C, D, 1), x, n_probe=2)
    new._cell_centres_dev[0, 5] = float('nan')
    ops.ivf_flat_centred_norms(new._vectors, new._cell_centres_dev, new._cell_of, n=new._n_rows, out=new._cell_cnorms)
    assert bool(new._cell_cnorms[:len(x)][new._cell_of[:len(x)] == 0].isnan().all())
    probes0 = int((_probed(new, q, 2)[2] == 0).any(dim=1).sum().item())
    assert probes0 >= 1
    _same(new.search_batch(q, limit=10), ref.search_batch(q, limit=10), 'NaN in the snapshot')
    assert new.last_overflowed == probes0 and ref.last_overflowed == 0


# ---- 7. dump / load ----------------------------------------------------------------------------------------------------------------------
def test_dump_and_load_carry_the_centres(ops, offset, tmp_path):
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex
    from annlite_amd.enums import Metric

    x, q, codebook = offset
    vq = _offset_vq(codebook)
    ref, new = _pair(1, 32, vq, x, n_probe=1)
    want = ref.search_batch(q, limit=10)
    new.dump(tmp_path / 'split.idx'), ref.dump(tmp_path / 'f32.idx')
    moved = _offset_vq((codebook + F(0.25)).astype(F))  # a codebook that moved since: the file's centres win

    def load(f, vq_codec=vq, **kw):
        return IvfFlatGpuIndex(32, vq_codec=vq_codec, n_probe=1, metric=Metric.EUCLIDEAN, index_file=tmp_path / f, **kw)

    back = load('split.idx', vq_codec=moved, cell_filter='bf16x3')
    assert np.array_equal(back.cell_centres_, codebook)
    assert np.array_equal(back._cell_cnorms[:len(x)].cpu().numpy(), new._cell_cnorms[:len(x)].cpu().numpy())
    back.vq_codec = vq  # (the selection reads the codec: the same cells as `ref` probes)
    _same(back.search_batch(q, limit=10), want, 'loaded with its centres')
    assert back.last_cell_filter == 'bf16x3' and back.last_overflowed == 0
    old = load('f32.idx', cell_filter='bf16x3')  # a file without the key: the codebook
    assert np.array_equal(old.cell_centres_, codebook)
    _same(old.search_batch(q, limit=10), want, 'a default index\'s file')
    assert old.last_cell_filter == 'bf16x3' and old.last_overflowed == 0
    plain = load('split.idx')  # ... and the key does not trouble a default index
    _same(plain.search_batch(q, limit=10), want, 'default index, file with centres')
    assert plain.cell_centres_ is None and plain.last_cell_filter == 'f32' and plain.last_overflowed == 50
