"""The int8 row store of the exact float search on the GPU ("int8 rows"): the i8 MFMA's operand map on exact
integer data; ``dtype=np.int8`` returns, bit for bit, what the f32 index returns over the rows ``s * clip(rint(x / s), -127, 127)``; at
the stage level every row within the bound is listed and the measured error stays inside the derived slack; non-finite and extreme
inputs keep the convention; a scale of one's own; update, growth, dump / load across the dtypes; the facade."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

F = np.float32
I8 = np.int8


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def codes(x, s):
    """f32 -> the int8 codes the index stores: clamp(rne(x / s), -127, 127), NaN -> 0"""
    with np.errstate(over='ignore', invalid='ignore'):
        t = np.asarray(x, dtype=F) * F(1.0 / s)  # (exact: s is a power of two)
        return np.clip(np.rint(np.nan_to_num(t, nan=0.0, posinf=127.0, neginf=-127.0)), -127, 127).astype(I8)


def stored(x, s):
    """the rows an int8 index of scale s stands for, as f32"""
    return (F(s) * codes(x, s).astype(F)).astype(F)


def default_scale(metric):
    return 2.0 ** -7 if metric == 3 else 1.0


def _index(metric, D, x, **kw):
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.enums import Metric

    kw.setdefault('initial_size', max(len(x), 1))
    idx = FlatGpuIndex(D, metric=Metric(metric), **kw)
    idx.add_with_ids(x, np.arange(len(x)))
    return idx


def _pair(metric, D, x, q, **kw):
    """(the int8 index over x, the f32 index that holds what it stores, the queries for either).  COSINE: an INNER_PRODUCT f32 index
    over the host-normalised-then-quantised rows, asked with the host-normalised queries -- a COSINE f32 index would normalise the
    quantised rows again."""
    from annlite_amd.math import l2_normalize_host

    new = _index(metric, D, x, dtype=np.int8, **kw)
    s = new.int8_scale_
    if metric == 3:
        with np.errstate(invalid='ignore', divide='ignore'):
            return new, _index(2, D, stored(l2_normalize_host(x), s)), l2_normalize_host(q)
    return new, _index(metric, D, stored(x, s)), q


def _same(got, want, what):
    (gd, gi), (wd, wi) = got, want
    assert gi.dtype == np.int64 and gd.dtype == np.float32
    assert np.array_equal(gi, wi), (what, np.argwhere(gi != wi)[:5], gi[gi != wi][:5], wi[gi != wi][:5])
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), (what, 'distance bits')


# ---- 1. the i8 MFMA's operand map: exact integer data, an asymmetric B ------------------------------------------------------------------
@pytest.mark.parametrize('D', [5, 32, 40, 96])
def test_filter_scores_of_integer_data_are_exact(ops, D):
    import torch

    N, B = 300, 130  # (3 row tiles, 2 query tiles, both with a ragged edge; D = 40: a K step that is three quarters padding; 96: two stages)
    r, j, b = np.arange(N)[:, None], np.arange(D)[None, :], np.arange(B)[:, None]
    x = ((r * 7 + j * 3) % 11 - 5).astype(F)
    q = ((b * 5 + j * j + b * j) % 13 - 6).astype(F)  # (not symmetric in (row, coordinate): a swapped operand or tile shows)
    q[:, 0] = 6  # (every query's largest value: one power of two, 2^17.  Q = 8 q 2^14: only the d2 plane is non-zero HERE -- the operand
    # map and the C tile; the next test puts data through all three planes and pins the rounding of the query)
    xd, qd = ops.to_dev(x.astype(I8)), ops.to_dev(q)
    for scale in (1.0, 0.25):  # (0.25: the scale folded into the query's power of two, rows a quarter as large)
        xs = (F(scale) * x).astype(F)
        norms = ops.flat_row_norms_i8(xd, scale)
        assert np.array_equal(norms.cpu().numpy(), (xs * xs).sum(1))
        bound = ops.to_dev(np.full(B, np.inf, F))
        for metric in (1, 2):
            cand, count, qn, qs, scores = ops.flat_filter_i8(metric, qd, xd, norms, bound, scale, scores=True)
            torch.cuda.synchronize()
            dot = q.astype(np.float64) @ xs.astype(np.float64).T
            want = ((xs * xs).sum(1)[None, :] + (q * q).sum(1)[:, None] - 2 * dot) if metric == 1 else 1 - dot
            assert np.array_equal(want.astype(F).astype(np.float64), want)  # (small integers and quarters: the f32 score is exact)
            assert np.array_equal(scores.cpu().numpy(), want.astype(F)), (metric, D, scale)
            assert np.array_equal(qn.cpu().numpy(), (q * q).sum(1)) and (count.cpu().numpy() == N).all()
            # max |q| = 6: E = 20 - 3 = 17 = e + log2 scale, and the per-query term is 1.001 * 127 * D * 2^-e
            e = 17 - int(np.log2(scale))
            assert np.allclose(qs.cpu().numpy(), 1.001 * 127 * D * 2.0 ** -e, rtol=1e-6, atol=0)
            assert np.array_equal(np.sort(cand.cpu().numpy()[:, :N], axis=1), np.tile(np.arange(N, dtype=np.int32), (B, 1)))


def _split_queries(B, D, E, rs):
    """Queries whose q' = q 2^E is known exactly: coordinate 0 is (2^19 + 5) +- 7/16 (the largest: it fixes E, and above 2^19 the f32 grid is
    2^-4), the others n + f with |n| < 2^16 and f a multiple of 1/32 drawn from values that tell the roundings apart -- 15/32 and 17/32
    either side of a tie, the ties themselves (to even: n odd and n even both occur), a quarter, none."""
    n = rs.randint(-2 ** 16, 2 ** 16, size=(B, D)).astype(np.float64)
    f = rs.choice([15 / 32, -15 / 32, 17 / 32, -17 / 32, 0.5, -0.5, 0.25, -0.25, 0.0], size=(B, D))
    n[:, 0], f[:, 0] = 2 ** 19 + 5, rs.choice([7 / 16, -7 / 16], size=B)
    qp = n + f
    q = (qp * 2.0 ** -E).astype(F)
    assert np.array_equal(q.astype(np.float64) * 2.0 ** E, qp)  # (every q' is an f32 number)
    return q, qp


def _digits(Q):
    d0 = ((Q + 64) & 127) - 64
    Q1 = (Q - d0) >> 7
    d1 = ((Q1 + 64) & 127) - 64
    return d0, d1, (Q1 - d1) >> 7


@pytest.mark.parametrize('D', [5, 32, 40, 96])
def test_filter_scores_use_all_three_digit_planes_and_the_query_rounded_to_nearest_even(ops, D):
    """The score the kernel must give is computable exactly: T = sum rint(q'_j) c_j is an integer, fl(T), the scaling by a power of two,
    fl(|x|^2 + |q|^2) on the norms the call returns and the last subtraction are single f32 roundings.  Q has all three digits non-zero, so
    the weights 2^14 / 2^7 / 1 of the recombination count; q' has a known fractional part, ties included, so a truncated or
    half-away-from-zero Q gives other scores."""
    import torch

    N, B, E = 300, 130, 12  # (q' = q 2^12: queries up to 128, next to rows of -5 .. 5)
    rs = np.random.RandomState(40 + D)
    r, j = np.arange(N)[:, None], np.arange(D)[None, :]
    c = ((r * 7 + j * 3) % 11 - 5).astype(np.int64)
    q, qp = _split_queries(B, D, E, rs)
    Q = np.rint(qp).astype(np.int64)  # (to nearest, ties to even)
    d0, d1, d2 = _digits(Q)
    assert np.array_equal(d2 * 16384 + d1 * 128 + d0, Q)
    assert (d0 != 0).mean() > 0.75 and (d1 != 0).mean() > 0.75 and (d2[:, 1:] != 0).mean() > 0.75 and (np.abs(d2[:, 0]) == 32).all()
    xd, qd = ops.to_dev(c.astype(I8)), ops.to_dev(q)
    bound = ops.to_dev(np.full(B, np.inf, F))

    def predicted(Qi, a, scale, metric):
        T = Qi @ c.T  # int64, exact
        dot = (T.astype(F) * F(scale * 2.0 ** -E)).astype(F)  # one conversion (numpy's is to nearest even too), an exact scaling
        return (a - F(2) * dot).astype(F) if metric == 1 else (F(1) - dot).astype(F)

    for scale in (1.0, 0.25):
        norms = ops.flat_row_norms_i8(xd, scale)
        assert np.array_equal(norms.cpu().numpy(), (F(scale) * c.astype(F) ** 2 * F(scale)).sum(1))
        for metric in (1, 2):
            cand, count, qn, qs, scores = ops.flat_filter_i8(metric, qd, xd, norms, bound, scale, scores=True)
            torch.cuda.synchronize()
            a = (norms.cpu().numpy()[None, :] + qn.cpu().numpy()[:, None]).astype(F)  # as the kernel adds them
            got = scores.cpu().numpy()
            want = predicted(Q, a, scale, metric)
            assert np.array_equal(got, want), (metric, D, scale, np.argwhere(got != want)[:5])
            # ... and the check tells the roundings apart: other integers next to q' (truncated, floored, halves up, halves away from
            # zero) give other scores -- in a third of the pairs and more under INNER_PRODUCT; under EUCLIDEAN, where |q|^2 near 10^4
            # D sits in the same f32 number, in fewer, at least 3 in 100
            for other in (np.trunc(qp), np.floor(qp), np.floor(qp + 0.5), np.where(qp >= 0, np.floor(qp + 0.5), np.ceil(qp - 0.5))):
                assert (predicted(other.astype(np.int64), a, scale, metric) != want).mean() > (0.03 if metric == 1 else 0.3)
            # ... as do the weights of the digits: a plane dropped or two planes swapped
            for wrong in (d2 * 16384 + d1 * 128, d2 * 16384 + d0, d1 * 16384 + d2 * 128 + d0, d2 * 16384 + d0 * 128 + d1):
                assert (predicted(wrong, a, scale, metric) != want).mean() > 0.9
            assert np.allclose(qs.cpu().numpy(), 1.001 * 127 * D * scale * 2.0 ** -E, rtol=1e-6, atol=0) and (count.cpu().numpy() == N).all()


# ---- 2. the same answer, bit for bit ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [4097, 4225, 12000])  # the filter engages above 4096 rows; a tile is 128 rows: 1 row, 1 tile + 1, many
@pytest.mark.parametrize('D', [1, 5, 31, 32, 33, 64, 130])
def test_i8_index_gives_the_f32_index_over_the_quantised_rows_its_bits(ops, D, N):
    import torch

    rs = np.random.RandomState(1000 * D + N % 997)
    x = (30 * rs.randn(N, D)).astype(F)
    x[7, 0], x[8, D - 1] = 500.0, -1e4  # (saturate whatever the draw)
    x[100:140] = x[100]  # a block of identical rows: ties ordered by id
    q = (30 * rs.randn(129, D)).astype(F)
    gone = np.arange(0, N, 3)
    keep = np.arange(1, N, 5)
    for metric in (1, 2, 3):
        qm = q.copy()
        new, ref, qr = _pair(metric, D, x, qm)
        s = new.int8_scale_
        assert s == default_scale(metric)
        held = ref._vectors[:N].cpu().numpy()
        qm[0] = held[100]  # a query equal to a stored value
        if metric == 3:
            from annlite_amd.math import l2_normalize_host
            qr = l2_normalize_host(qm)
        else:
            qr = qm
        assert new._vectors.dtype == torch.int8 and ref._vectors.dtype == torch.float32 and new.flat_filter == 'i8x3'
        got_codes = new._vectors[:N].cpu().numpy()
        assert got_codes.dtype == I8 and np.array_equal(got_codes, codes(held, s)) and np.array_equal(held, F(s) * got_codes.astype(F))
        assert np.abs(got_codes).max() == 127 and got_codes.min() >= -127
        for B in (1, 129):
            for k in (1, 10, 64, 100):
                got, want = new.search_batch(qm[:B], limit=k), ref.search_batch(qr[:B], limit=k)
                _same(got, want, (metric, B, k))
                ran = k <= 64 or N > 2 * ops.flat_list_capacity()  # (limit > 64 on a small table: exact sums over all rows, no filter)
                assert new.last_flat_filter == ('i8x3' if ran else None) and ref.last_flat_filter == ('f32' if ran else None)
                # a condition, not a tolerance: where the f32 filter's lists hold, the int8 filter's must hold as well
                if ref.last_overflowed == 0 and D >= 16:
                    assert new.last_overflowed == 0, (metric, B, k, new.last_overflowed)
                if metric == 1:  # the rows that equal the query come first, at distance 0, by id (at small D other rows share the codes)
                    twins = np.nonzero((held == held[100]).all(1))[0][:k]
                    assert len(twins) >= min(k, 40) and np.isin(np.arange(100, 140), np.nonzero((held == held[100]).all(1))[0]).all()
                    assert (got[0][0, :len(twins)] == 0.0).all() and list(got[1][0, :len(twins)]) == list(twins)
        _same(new.search_batch(qm, limit=10, indices=keep), ref.search_batch(qr, limit=10, indices=keep), (metric, 'a fifth kept'))
        assert new.last_flat_filter == 'i8x3' and (ref.last_overflowed > 0 or D < 16 or new.last_overflowed == 0)
        for idx in (ref, new):
            idx.delete(gone)
        for B, k in ((129, 10), (1, 64), (5, 100)):
            _same(new.search_batch(qm[:B], limit=k), ref.search_batch(qr[:B], limit=k), (metric, B, k, 'a third deleted'))
            assert new.last_flat_filter == ('i8x3' if k <= 64 or N > 2 * ops.flat_list_capacity() else None)
            assert ref.last_overflowed > 0 or D < 16 or new.last_overflowed == 0


# ---- 3. the stage alone: a superset, and the measured error ---------------------------------------------------------------------------
@pytest.mark.parametrize('metric', [1, 2])
@pytest.mark.parametrize('D', [16, 130])
@pytest.mark.parametrize('scale', [1.0, 2.0 ** -7])
def test_stage_lists_every_row_within_the_bound(ops, scale, D, metric):
    import torch
    from annlite_amd.core.index.row_store import RowStoreIndex

    N, B, k = 5000, 8, 50
    rs = np.random.RandomState(17 * D + metric)
    c = codes(30 * rs.randn(N, D), 1.0)
    x = (F(scale) * c.astype(F)).astype(F)
    q = (scale * 30 * rs.randn(B, D)).astype(F)
    q[0] = x[7]                                     # a stored row
    q[1] = x[9] * F(1 + 2 ** -20) + F(scale * 0.49)  # next to one, every coordinate just short of a tie of the query's rounding
    q[2] *= F(1e-3)                                 # small against the rows
    q[3] *= F(1e3)                                  # large against them
    xd, qd = ops.to_dev(c), ops.to_dev(q)
    flags = torch.ones(((N + 31) // 32 + 2) * 32, dtype=torch.bool, device=xd.device)
    flags[N:] = False
    flags[torch.arange(3, N, 7, device=xd.device)] = False
    bits = RowStoreIndex._pack_bits(flags)
    ok = flags[:N].cpu().numpy()
    norms = ops.flat_row_norms_i8(xd, scale)
    assert np.array_equal(norms.cpu().numpy().view(np.uint32), ops.flat_row_norms(ops.to_dev(x)).cpu().numpy().view(np.uint32))
    rows = torch.arange(N, dtype=torch.int64, device=xd.device)[None, :].expand(B, N).contiguous()
    exact = ops.exact_gather_dist_i8(metric, qd, xd, rows, scale).cpu().numpy()  # the arithmetic of the search's exact stage
    assert np.array_equal(exact.view(np.uint32), ops.exact_gather_dist(metric, qd, ops.to_dev(x), rows).cpu().numpy().view(np.uint32))
    bound = np.sort(np.where(ok[None, :], exact, np.inf), axis=1)[:, k - 1].astype(F)  # the 50th smallest true score
    cand, count, qn, qs, scores = ops.flat_filter_i8(metric, qd, xd, norms, ops.to_dev(bound), scale, valid_bits=bits, scores=True)
    torch.cuda.synchronize()
    cand, count, qn, qs, scores, norms = (t.cpu().numpy() for t in (cand, count, qn, qs, scores, norms))
    c_rel, c_abs = ops.flat_i8_slack(metric, D)
    q64, x64 = q.astype(np.float64), x.astype(np.float64)
    # the per-query term: 1.001 * 127 * D * 2^-e, 2^-e = scale / 2^E, max |q| 2^E in [2^19, 2^20)
    two_E = 2.0 ** (20 - np.frexp(np.abs(q).max(1))[1])
    assert np.allclose(qs, 1.001 * 127 * D * scale / two_E, rtol=1e-6, atol=0)
    slack32 = ((F(c_rel) * (norms[None, :N] + qn[:, None]).astype(F) + F(c_abs)).astype(F) + qs[:, None]).astype(F)  # as the kernel adds it
    slack = slack32.astype(np.float64)
    d64 = ((x64[None] - q64[:, None]) ** 2).sum(-1) if metric == 1 else 1.0 - q64 @ x64.T
    assert np.isfinite(scores).all() and scores.shape == (B, N)
    worst = 0.0
    for b in range(B):
        assert 0 < count[b] <= ops.flat_list_capacity()
        lst = cand[b, :count[b]]
        assert len(set(lst.tolist())) == len(lst), 'a row listed twice'
        assert ((lst >= 0) & (lst < N)).all() and ok[lst].all(), 'an invalid row listed'
        need = np.nonzero(ok & (exact[b] <= bound[b]))[0]
        assert len(need) >= k and np.isin(need, lst).all(), (b, 'a row within the bound is missing')
        assert (d64[b, lst] <= float(bound[b]) + 2 * slack[b, lst]).all(), 'a listed row lies beyond the bound by more than twice the slack'
        # ... and the kernel's comparison, redone on its own scores, is the list
        passed = np.nonzero(ok & ~(scores[b] > (bound[b] + slack32[b]).astype(F)))[0]
        assert np.array_equal(np.sort(lst), passed)
        ratio = (np.abs(scores[b].astype(np.float64) - d64[b]) / slack[b])[ok]  # (a row that is not valid is scored without its norm)
        print(f'int8 filter |v - d| / slack: scale={scale} D={D} metric={metric} query {b}: worst={ratio.max():.4f} listed={count[b]}')
        worst = max(worst, float(ratio.max()))
    assert worst <= 1.0  # (the derived slack covers the measured error of every pair)


# ---- 4. small tables ----------------------------------------------------------------------------------------------------------------------
def test_small_tables_run_no_filter(ops):
    rs = np.random.RandomState(2)
    x, q = (30 * rs.randn(4096, 16)).astype(F), (30 * rs.randn(3, 16)).astype(F)
    small, ref = _index(1, 16, x, dtype='int8'), _index(1, 16, stored(x, 1.0))
    for k in (10, 100):
        _same(small.search_batch(q, limit=k), ref.search_batch(q, limit=k), ('4096 rows', k))
        assert small.last_flat_filter is None and small.last_overflowed == 0


# ---- 5. non-finite and extreme inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', [1, 2, 3])
def test_non_finite_and_extreme_inputs_answer_as_the_f32_index_over_the_stored_rows(ops, metric):
    rs = np.random.RandomState(9)
    x, q = (30 * rs.randn(5000, 16)).astype(F), (30 * rs.randn(9, 16)).astype(F)
    q[1, 3], q[2, 0], q[3, 15], q[4, :], q[5, :], q[6, :], q[7, :] = np.nan, np.inf, -np.inf, np.nan, 0.0, 1e30 * q[6], 1e-30 * q[7]
    x[77, 5], x[78, 6], x[4999, 0], x[4998, 1], x[12, :] = np.nan, 1e9, np.inf, -np.inf, 0.0
    new, ref, qr = _pair(metric, 16, x, q)
    got_codes = new._vectors[:5000].cpu().numpy()
    if metric != 3:  # (COSINE normalises first: a row with a NaN or an infinity is all NaN after that, all zero in the store)
        assert got_codes[77, 5] == 0 and got_codes[78, 6] == 127 and got_codes[4999, 0] == 127 and got_codes[4998, 1] == -127
    else:
        assert not got_codes[77].any() and not got_codes[4999].any() and not got_codes[4998].any() and got_codes[78, 6] == 127
    assert got_codes.min() >= -127 and np.array_equal(got_codes, codes(ref._vectors[:5000].cpu().numpy(), new.int8_scale_))
    for k in (1, 10, 64, 100):
        want, got = ref.search_batch(qr, limit=k), new.search_batch(q, limit=k)
        _same(got, want, (metric, k))
        # the NaN and +-inf queries (1 .. 4) have no integer planes: every row passes, their lists overflow
        assert k > 64 or (new.last_flat_filter == 'i8x3' and new.last_overflowed >= 4)  # (limit 100, 5000 rows: no filter runs)
        print(f'non-finite inputs: metric={metric} k={k} overflowed int8={new.last_overflowed} f32={ref.last_overflowed}')


# ---- 6. a scale of one's own ------------------------------------------------------------------------------------------------------------
def test_a_scale_other_than_the_default(ops):
    rs = np.random.RandomState(12)
    N, D, s = 4225, 33, 2.0 ** -3
    x, q = (4 * rs.randn(N, D)).astype(F), (4 * rs.randn(129, D)).astype(F)  # (4 / s = 32 code steps per sigma: some rows saturate)
    x[100:140] = x[100]
    new, ref = _index(1, D, x, dtype=np.int8, int8_scale=s), _index(1, D, stored(x, s))
    q[0] = stored(x[100], s)
    assert new.int8_scale_ == s and np.array_equal(new._vectors[:N].cpu().numpy(), codes(x, s)) and np.abs(codes(x, s)).max() == 127
    for B, k in ((129, 10), (1, 64), (129, 100), (1, 1)):
        got = new.search_batch(q[:B], limit=k)
        _same(got, ref.search_batch(q[:B], limit=k), (B, k))
        assert new.last_flat_filter == ('i8x3' if k <= 64 else None) and (ref.last_overflowed > 0 or new.last_overflowed == 0)
        assert got[0][0, 0] == 0.0 and got[1][0, 0] == 100
    keep = np.arange(1, N, 5)
    _same(new.search_batch(q, limit=10, indices=keep), ref.search_batch(q, limit=10, indices=keep), 'a fifth kept')
    assert new.last_flat_filter == 'i8x3' and (ref.last_overflowed > 0 or new.last_overflowed == 0)
    for idx in (ref, new):
        idx.delete(np.arange(0, N, 3))
    for B, k in ((129, 10), (1, 64), (5, 100)):
        _same(new.search_batch(q[:B], limit=k), ref.search_batch(q[:B], limit=k), (B, k, 'a third deleted'))
        assert new.last_flat_filter == ('i8x3' if k <= 64 else None) and (ref.last_overflowed > 0 or new.last_overflowed == 0)


# ---- 7. lifecycle -----------------------------------------------------------------------------------------------------------------------
def test_updated_rows_are_quantised_again_and_carry_their_norms(ops):
    rs = np.random.RandomState(4)
    x = (30 * rs.randn(6000, 33)).astype(F)
    new, ref = _index(1, 33, x, dtype=np.int8), _index(1, 33, stored(x, 1.0))
    ids = rs.choice(6000, 100, replace=False)
    moved = (80.0 + 10 * rs.randn(100, 33)).astype(F)  # far from where the rows were: a stale norm would put the filter's score far off
    new.update_with_ids(moved, ids)
    ref.update_with_ids(stored(moved, 1.0), ids)
    assert np.array_equal(new._vectors[ids].cpu().numpy(), codes(moved, 1.0))
    assert np.array_equal(new._norms[:6000].cpu().numpy().view(np.uint32), ref._norms[:6000].cpu().numpy().view(np.uint32))
    q = np.concatenate([stored(moved[:20], 1.0), (30 * rs.randn(5, 33)).astype(F)])
    got = new.search_batch(q, limit=10)
    _same(got, ref.search_batch(q, limit=10), 'after update_with_ids')
    assert np.array_equal(got[1][:20, 0], ids[:20]) and (got[0][:20, 0] == 0.0).all() and new.last_overflowed == 0


def test_dump_and_load_across_the_dtypes(ops, tmp_path):
    import torch
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.enums import Metric

    rs = np.random.RandomState(6)
    s = 0.5
    x, q = (10 * rs.randn(5000, 32)).astype(F), (10 * rs.randn(7, 32)).astype(F)
    byte, full, ref = _index(1, 32, x, dtype=np.int8, int8_scale=s), _index(1, 32, x), _index(1, 32, stored(x, s))
    for idx in (byte, full, ref):
        idx.delete([5, 4000])
    want, want_full = ref.search_batch(q, limit=10), full.search_batch(q, limit=10)
    byte.dump(tmp_path / 'i8.bin'), full.dump(tmp_path / 'f32.bin')
    state = np.load(tmp_path / 'i8.bin', allow_pickle=True)[0]
    assert state['format'] == FlatGpuIndex.FORMAT and state['vectors'].dtype == I8 and state['int8_scale'] == s  # (one format)
    assert np.array_equal(state['vectors'], codes(x, s))
    assert 'int8_scale' not in np.load(tmp_path / 'f32.bin', allow_pickle=True)[0]
    for file, kw, expect in (('i8.bin', dict(dtype=np.int8, int8_scale=s), want),    # the codes as they are
                             ('f32.bin', dict(dtype=np.int8, int8_scale=s), want),   # floats are quantised with the index's scale
                             ('i8.bin', dict(dtype=np.float32), want),               # codes are widened with the file's scale
                             ('i8.bin', dict(dtype=np.float16), want),               # (|s c| <= 63.5 in steps of 0.5: exact in f16)
                             ('f32.bin', dict(dtype=np.float32), want_full)):
        back = FlatGpuIndex(32, metric=Metric.EUCLIDEAN, index_file=tmp_path / file, **kw)
        kind = np.dtype(kw['dtype'])
        assert back._vectors.dtype == {'int8': torch.int8, 'float16': torch.float16, 'float32': torch.float32}[kind.name] and back.size == 4998
        if kind == np.int8:
            assert np.array_equal(back._vectors[:5000].cpu().numpy(), codes(x, s))
        elif expect is want:
            assert np.array_equal(back._vectors[:5000].cpu().numpy().astype(F), stored(x, s))  # the values s c
        _same(back.search_batch(q, limit=10), expect, (file, kw))
        assert back.last_flat_filter == {'int8': 'i8x3', 'float16': 'f16x2', 'float32': 'f32'}[kind.name] and back.last_overflowed == 0
        _same(back.search_batch(q, limit=70), (ref if expect is want else full).search_batch(q, limit=70), (file, kw, 'limit 70'))
        assert np.array_equal(back._norms[:5000].cpu().numpy(), (ref if expect is want else full)._norms[:5000].cpu().numpy())
    with pytest.raises(ValueError, match=r'int8_scale=0\.5.*int8_scale=1\.0'):  # codes of one scale are not codes of another
        FlatGpuIndex(32, dtype=np.int8, metric=Metric.EUCLIDEAN, index_file=tmp_path / 'i8.bin')


def test_growth_past_the_initial_size_and_reset(ops):
    import torch

    rs = np.random.RandomState(7)
    x, q = (30 * rs.randn(5000, 24)).astype(F), (30 * rs.randn(9, 24)).astype(F)
    new = _index(2, 24, x[:700], dtype=np.int8, initial_size=1000, expand_step_size=1000)
    for lo in range(700, 5000, 900):
        new.add_with_ids(x[lo:lo + 900], np.arange(lo, min(lo + 900, 5000)))
    assert new.capacity == 5000 and new.size == 5000 and new._vectors.dtype == torch.int8 and new._vectors.shape == (5000, 24)
    assert np.array_equal(new._vectors.cpu().numpy(), codes(x, 1.0))  # (every growth copied the bytes)
    _same(new.search_batch(q, limit=10), _index(2, 24, stored(x, 1.0)).search_batch(q, limit=10), 'grown')
    new.reset()
    assert new.size == 0 and new._vectors is None
    new.add_with_ids(x[:10], np.arange(10))
    assert new._vectors.dtype == torch.int8


# ---- 8. the facade ------------------------------------------------------------------------------------------------------------------------
def test_facade_over_int8_rows_equals_the_facade_over_the_quantised_rows(ops, tmp_path):
    from annlite_amd import AnnLite
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.docarray_compat import Document, DocumentArray

    rs = np.random.RandomState(23)
    N, D = 4500, 24
    x, q = (30 * rs.randn(N, D)).astype(F), (30 * rs.randn(20, D)).astype(F)
    moved = (30 * rs.randn(50, D)).astype(F)
    new = AnnLite(D, dtype=np.int8, metric='euclidean', data_path=str(tmp_path / 'i8'))
    ref = AnnLite(D, metric='euclidean', data_path=str(tmp_path / 'f32'))
    for ann, rows, upd in ((new, x, moved), (ref, stored(x, 1.0), stored(moved, 1.0))):
        ann.index(DocumentArray([Document(id=str(i), embedding=rows[i], tags={'g': int(i % 3)}) for i in range(N)]))
        ann.delete([str(i) for i in range(0, N, 7)])
        ann.update(DocumentArray([Document(id=str(i), embedding=upd[n], tags={'g': int(i % 3)}) for n, i in enumerate(range(1, 351, 7))]))
    idx = new.vec_index(0)
    assert type(idx) is FlatGpuIndex and idx._i8 and idx.int8_scale_ == 1.0 and new.index_size == ref.index_size == N - len(range(0, N, 7))

    def answers(ann, **kw):
        dists, ids = ann.search_numpy(q, limit=10, **kw)
        return np.stack(dists).astype(F), np.stack(ids).astype(np.int64)

    _same(answers(new), answers(ref), 'search_numpy')
    assert idx.last_flat_filter == 'i8x3' and idx.last_overflowed == 0
    _same(answers(new, filter={'g': {'$eq': 1}}), answers(ref, filter={'g': {'$eq': 1}}), 'filter')
    new.dump()
    again = AnnLite(D, dtype=np.int8, metric='euclidean', data_path=str(tmp_path / 'i8'))
    back = again.vec_index(0)
    assert type(back) is FlatGpuIndex and back._i8 and again.index_size == new.index_size
    assert np.array_equal(back._vectors[:back._n_rows].cpu().numpy(), idx._vectors[:idx._n_rows].cpu().numpy())
    _same(answers(again), answers(ref), 'reopened')
