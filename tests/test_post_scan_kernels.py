"""The kernels BEHIND the scan (scan.hip), each against the oracle or numpy written here, at the shapes and values the end-to-end
tests never hand them: ``topk_rows_kernel`` / ``math.top_k``, ``merge_lists_kernel`` (plain and packed), ``adc_dist_kernel``,
``adc_gather_kernel``, ``codes_skew_kernel``, and ``seed_union_kernel`` as a property of the search it feeds.

Order rule everywhere: numpy's (``math.py:94-120`` selects with argpartition / argsort) -- -0.0 == +0.0, every NaN behind +inf
whatever its sign bit and payload -- with ties by id (``oracle/pq_oracle.c: pair_less``).  Values are compared with
``array_equal`` (under which the two zeros agree; ``equal_nan`` where NaN is an input), ids exactly.

The numpy restatements used as references (NaN-last lexsort, the SKEWED layout incl. the M = 64 wrap coding) are themselves
checked on the CPU, against the oracle or a brute-force loop, at the top of the file."""
import numpy as np
import pytest

from _refs import NANS, SUBNORMALS, bits as _bits, f32_key, lexsort_nan_last, on_gpu, skew_rows, topk_pairs, topk_pairs_numpy


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _skew_loop(plain, ids):
    """brute force, one byte at a time, straight from the sentence in DESIGN section 2"""
    N, M = plain.shape
    out = np.zeros_like(plain)
    for i in range(N):
        n = int(ids[i])
        for j in range(M):
            if M == 64:
                h, p, r = j // 32, j % 32, n % 32
                out[i, j] = (int(plain[i, 32 * h + (p + r) % 32]) - (1 if p + r >= 32 else 0)) % 256
            else:
                out[i, j] = plain[i, (j + n) % M]
    return out


def _wrap_rows(rs, n, M):
    """random code rows; for M = 64 every fourth row all 0, every fourth all 255: the -1 / +1 of the wrap coding passes through
    both ends of the byte at every wrap position"""
    c = rs.randint(0, 256, size=(n, M)).astype(np.uint8)
    c[0::4] = 0
    c[1::4] = 255
    return c


# ------------------------------------------------------------------------------------------- CPU: the references themselves
def _value_rows(rs, N):
    """rows of N floats that a selection can get wrong: see the names"""
    rows = {}
    rows['random'] = rs.randn(N).astype(np.float32)
    rows['ties'] = rs.randint(0, 4, size=N).astype(np.float32)
    rows['all_equal'] = np.full(N, 2.5, np.float32)
    rows['all_inf'] = np.full(N, np.inf, np.float32)
    rows['all_nan'] = NANS[rs.randint(0, NANS.size, size=N)]
    rows['mixed_nonfinite'] = np.concatenate([_bits(0x7f800000, 0xff800000), NANS, rs.randn(3).astype(np.float32)])[
        rs.randint(0, 11, size=N)]
    rows['signed_nans_first'] = np.where(np.arange(N) % 3 == 0, NANS[1], rs.randn(N).astype(np.float32))
    rows['zeros_neg_first'] = _bits(0x80000000, 0x00000000)[np.arange(N) % 2]      # [-0.0 (id 0), +0.0 (id 1), ...]
    rows['zeros_pos_first'] = _bits(0x00000000, 0x80000000)[np.arange(N) % 2]      # [+0.0 (id 0), -0.0 (id 1), ...]
    rows['zeros_among_numbers'] = np.concatenate([_bits(0x00000000, 0x80000000), np.float32([1, -1])])[rs.randint(0, 4, size=N)]
    rows['subnormals'] = np.concatenate([SUBNORMALS, _bits(0x00000000, 0x80000000)])[rs.randint(0, 6, size=N)]
    return rows


def test_reference_lexsort_equals_the_oracle_and_a_brute_force_selection(oracle):
    rs = np.random.RandomState(0)
    for N in (1, 2, 7, 65):
        for name, v in _value_rows(rs, N).items():
            ids = np.arange(N) + 5
            o = lexsort_nan_last(v, ids)
            # brute force: selection sort under "a before b" = a is a number and (b is NaN or a < b), or tied and lower id
            def before(a, b):
                an, bn = np.isnan(v[a]), np.isnan(v[b])
                if an != bn:
                    return bn
                if not an and v[a] != v[b]:
                    return v[a] < v[b]
                return ids[a] < ids[b]
            left, want = list(range(N)), []
            while left:
                best = left[0]
                for c in left[1:]:
                    if before(c, best):
                        best = c
                want.append(best)
                left.remove(best)
            assert o.tolist() == want, (name, N)
            for k in (1, 3, N, N + 2):
                d, i = oracle.top_k_c(v, k, 5)
                d2, i2 = topk_pairs_numpy(v, ids, k)
                assert np.array_equal(i, i2) and np.array_equal(d, d2, equal_nan=True), (name, N, k)
                d3, i3 = topk_pairs(oracle, v[::-1], ids[::-1], k)  # pairs handed over in another order: the same answer
                assert np.array_equal(i, i3) and np.array_equal(d, d3, equal_nan=True), (name, N, k)


def test_reference_signed_zero_row_returns_the_lower_id(oracle):
    d, i = oracle.top_k_c(_bits(0x00000000, 0x80000000), 1)
    assert i[0] == 0 and d[0] == 0
    assert lexsort_nan_last(_bits(0x00000000, 0x80000000), [0, 1])[0] == 0


@pytest.mark.parametrize('M', [1, 3, 8, 16, 32, 64, 128])
def test_reference_skew_equals_the_byte_loop_and_inverts(M):
    rs = np.random.RandomState(M)
    n = 70
    plain = _wrap_rows(rs, n, M)
    ids = rs.permutation(500)[:n] + 3
    ids[:4] = [31, 32, 63, 64]
    st = skew_rows(plain, ids)
    assert np.array_equal(st, _skew_loop(plain, ids))
    assert np.array_equal(skew_rows(st, ids, inverse=True), plain)
    if M == 64:  # a row with id % 32 = 31: every position but the first of each half wraps; zeros are stored as 255
        z = skew_rows(np.zeros((1, 64), np.uint8), [31])[0]
        assert z[0] == 0 and z[32] == 0 and (z[1:32] == 255).all() and (z[33:] == 255).all()


# ------------------------------------------------------------------------------------------- GPU: topk_rows / math.top_k
def _matrix(rs, N):
    rows = _value_rows(rs, N)
    return list(rows), np.stack([rows[n] for n in rows])


@on_gpu
@pytest.mark.parametrize('N', [0, 1, 63, 64, 65, 4097])
def test_topk_rows_equals_the_oracle(ops, oracle, N):
    import torch

    rs = np.random.RandomState(N)
    names, v = _matrix(rs, N)
    assert v.shape[0] % 4 != 0  # B not a multiple of the four waves of a workgroup
    vd = ops.to_dev(v) if N else torch.empty((v.shape[0], 0), dtype=torch.float32, device=ops.device())
    for k in (1, 2, 16, 63, 64):
        for id_base in (0, (1 << 33) + 5):
            d, i = ops.topk_rows(vd, k, id_base=id_base)
            d, i = d.cpu().numpy(), i.cpu().numpy()
            for b, name in enumerate(names):
                wd, wi = oracle.top_k_c(v[b], k, id_base)
                wd2, wi2 = topk_pairs_numpy(v[b], np.arange(N, dtype=np.int64) + id_base, k)
                assert np.array_equal(wi, wi2) and np.array_equal(wd, wd2, equal_nan=True)
                assert np.array_equal(i[b], wi), (name, N, k, id_base, i[b][:8], wi[:8])
                assert np.array_equal(d[b], wd, equal_nan=True), (name, N, k, id_base)


@on_gpu
def test_topk_rows_signed_zero_pair_returns_id_0(ops):
    d, i = ops.topk_rows(ops.to_dev(_bits(0x00000000, 0x80000000).reshape(1, 2)), 1)
    assert int(i.cpu()[0, 0]) == 0 and float(d.cpu()[0, 0]) == 0.0


@on_gpu
@pytest.mark.parametrize('N', [1, 65, 300])
def test_math_top_k_descending_over_zeros_and_non_finite_rows(ops, oracle, N):
    """``descending=True`` negates on the way in: every +0.0 arrives as -0.0.  Both the wave kernel (k <= 64) and the device sort."""
    from annlite_amd import math as amath

    rs = np.random.RandomState(N + 1)
    names, v = _matrix(rs, N)
    for k in (1, 16, 64, 100):
        kk = min(k, N)
        for desc in (False, True):
            d, i = amath.top_k(v, k, descending=desc)
            assert d.shape == (v.shape[0], kk)
            for b, name in enumerate(names):
                wd, wi = oracle.top_k_c(-v[b] if desc else v[b], kk)
                assert np.array_equal(i[b], wi), (name, N, k, desc)
                assert np.array_equal(d[b], -wd if desc else wd, equal_nan=True), (name, N, k, desc)


@on_gpu
@pytest.mark.parametrize('dtype', [np.int32, np.int64, np.float64])
def test_math_top_k_takes_integer_and_float64_rows(ops, dtype):
    """Other dtypes than float32, on both paths (wave kernel up to k = 64, device sort above) and for N = 0: indices under (value,
    index), values equal to the input's."""
    from annlite_amd import math as amath

    rs = np.random.RandomState(np.dtype(dtype).itemsize)
    for N in (0, 1, 300):
        v = rs.randint(0, 40, size=(5, N)).astype(dtype)
        for k in (1, 64, 100, 450):
            kk = min(k, N)
            for desc in (False, True):
                d, i = amath.top_k(v, k, descending=desc)
                assert d.shape == (5, kk) and i.shape == (5, kk), (N, k, desc)
                w = -v.astype(np.int64) if desc else v.astype(np.int64)
                wi = np.stack([np.lexsort((np.arange(N), w[b]))[:kk] for b in range(5)]).reshape(5, kk)
                assert np.array_equal(i, wi), (dtype, N, k, desc)
                assert np.array_equal(d.astype(np.float64), np.take_along_axis(v, wi, axis=1).astype(np.float64)), (dtype, N, k, desc)


# ------------------------------------------------------------------------------------------- GPU: topk_merge / topk_merge_packed
def _shard_lists(rs, G, B, k, sqrt_safe):
    """[G, B, k] lists as the ranks of a row-sharded search hand them over: ascending in (distance, id), padding (+inf or
    anything, id -1) behind.  Per query a different situation; ids are global rows, distinct over the shards of a query."""
    pool = [np.float32(x) for x in (0.0, 1.0, 1.0, 2.5, np.inf)] + list(_bits(0x80000000, 0x00000000)) + list(NANS[:3])
    if not sqrt_safe:
        pool += [np.float32(-1.0), np.float32(-np.inf)] + list(SUBNORMALS)
    dist = np.full((G, B, k), np.inf, np.float32)
    ids = np.full((G, B, k), -1, np.int64)
    for b in range(B):
        perm = rs.permutation(G * k + 7)
        all_ids = np.where(perm % 3 == 0, perm + (1 << 33), perm).astype(np.int64)  # some above 2^32, some small
        mode = b % 6
        for g in range(G):
            n = k                                                  # full lists
            if mode == 1:
                n = rs.randint(0, k + 1)                            # some padding
            elif mode == 2:
                n = 1 if g == G - 1 else 0                          # one entry in all
            elif mode == 3:
                n = 0                                               # nothing: (+inf, -1)
            own = all_ids[g * k:g * k + n]
            if mode == 4:
                d = np.full(n, 1.0, np.float32)                     # every distance equal, in every shard: ids decide
            elif mode == 5:
                d = _bits(0x00000000, 0x80000000)[rs.randint(0, 2, size=n)]   # +-0.0 only
            else:
                d = np.array([pool[j] for j in rs.randint(0, len(pool), size=n)], np.float32)
                fin = rs.rand(n) < 0.4
                d[fin] = (rs.randint(0, 6, size=int(fin.sum())) / np.float32(2)).astype(np.float32)
            o = lexsort_nan_last(d, own)
            dist[g, b, :n], ids[g, b, :n] = d[o], own[o]
            if n < k and b % 2:
                dist[g, b, n:] = 0.25                                # a padding entry's distance is not looked at
    return dist, ids


def _merge_expected(oracle, dist, ids, k, sqrt):
    G, B, _ = dist.shape
    wd, wi = np.empty((B, k), np.float32), np.empty((B, k), np.int64)
    for b in range(B):
        d, i = dist[:, b].ravel(), ids[:, b].ravel()
        ok = i >= 0
        wd[b], wi[b] = topk_pairs(oracle, d[ok], i[ok], k)
        d2, i2 = topk_pairs_numpy(d[ok], i[ok], k)
        assert np.array_equal(wi[b], i2) and np.array_equal(wd[b], d2, equal_nan=True)
    if sqrt:
        with np.errstate(invalid='ignore'):
            wd = np.where(wi >= 0, np.sqrt(wd), wd)
    return wd, wi


@on_gpu
@pytest.mark.parametrize('G', [1, 2, 3, 8, 16])
@pytest.mark.parametrize('k', [1, 10, 50, 64])
def test_topk_merge_both_forms_equal_the_oracle(ops, oracle, G, k):
    rs = np.random.RandomState(100 * G + k)
    B = 13
    for sqrt in (False, True):
        dist, ids = _shard_lists(rs, G, B, k, sqrt_safe=sqrt)
        wd, wi = _merge_expected(oracle, dist, ids, k, sqrt)
        assert (wi[3] == -1).all() and np.isinf(wd[3]).all()       # the query without any entry
        for order in (np.arange(G), np.arange(G)[::-1]):           # the lower id wins whatever the shard order
            dg, ig = np.ascontiguousarray(dist[order]), np.ascontiguousarray(ids[order])
            packed = np.stack([ig, dg.view(np.uint32).astype(np.int64)], axis=-1)
            pd_, pi_ = ops.topk_merge_packed(ops.to_dev(packed), sqrt=sqrt)
            pd_, pi_ = pd_.cpu().numpy(), pi_.cpu().numpy()
            assert np.array_equal(pi_, wi), (G, k, sqrt, np.argwhere(pi_ != wi)[:3])
            assert np.array_equal(pd_, wd, equal_nan=True), (G, k, sqrt)
            if not sqrt:
                md, mi = ops.topk_merge(ops.to_dev(dg), ops.to_dev(ig))
                md, mi = md.cpu().numpy(), mi.cpu().numpy()
                assert np.array_equal(mi, wi), (G, k, np.argwhere(mi != wi)[:3])
                assert np.array_equal(md.view(np.uint32), pd_.view(np.uint32))  # the two forms agree bit for bit


@on_gpu
def test_topk_merge_packed_sqrt_of_zero_inf_nan_and_padding(ops):
    dist = np.array([[[0.0, 4.0, np.inf]], [[-0.0, np.nan, 9.0]]], np.float32)       # G = 2, B = 1, k = 3; 9.0 is padding
    ids = np.array([[[7, 3, 11]], [[5, 2, -1]]], np.int64)
    packed = np.stack([ids, dist.view(np.uint32).astype(np.int64)], axis=-1)
    d, i = ops.topk_merge_packed(ops.to_dev(packed), sqrt=True)
    assert i.cpu().numpy().tolist() == [[5, 7, 3]]
    assert np.array_equal(d.cpu().numpy(), np.float32([[0.0, 0.0, 2.0]]))
    packed6 = np.concatenate([packed, np.stack([np.full((2, 1, 3), -1, np.int64), np.zeros((2, 1, 3), np.int64)], -1)], axis=2)
    d, i = ops.topk_merge_packed(ops.to_dev(np.ascontiguousarray(packed6)), sqrt=True)  # k = 6: five entries, one (+inf, -1)
    assert i.cpu().numpy().tolist() == [[5, 7, 3, 11, 2, -1]]
    assert np.array_equal(d.cpu().numpy(), np.float32([[0.0, 0.0, 2.0, np.inf, np.nan, np.inf]]), equal_nan=True)


# ------------------------------------------------------------------------------------------- GPU: adc_dist / adc_gather
def _table(rs, M, Ks, nonfinite):
    t = rs.randn(M, Ks).astype(np.float32)
    if nonfinite:
        flat = t.reshape(-1)
        idx = rs.choice(flat.size, max(3, flat.size // 50), replace=False)
        flat[idx] = np.concatenate([_bits(0x7f800000, 0xff800000), NANS])[rs.randint(0, 8, size=idx.size)]
    return t


def _codes(rs, N, M, Ks, cb):
    c = rs.randint(0, Ks, size=(N, M)).astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[cb])
    c[0, :] = Ks - 1
    c[-1, :] = 0
    return c


ADC_SHAPES = [  # (M, Ks, code bytes): M * Ks * 4 <= 64 KiB -> the table sits in LDS, above -> read from global memory
    (1, 256, 1), (3, 100, 1), (16, 256, 1), (128, 256, 1),   # 128 * 256 * 4 = 128 KiB: global, uint8
    (16, 512, 2), (32, 1024, 2),                             # 32 KiB: LDS / 128 KiB: global, uint16
    (3, 300, 4), (16, 1025, 4),                              # LDS / 64.06 KiB: global (one entry over), uint32
    (16, 1024, 2),                                           # exactly 64 KiB: LDS
]


@on_gpu
@pytest.mark.parametrize('M,Ks,cb', ADC_SHAPES)
@pytest.mark.parametrize('nonfinite', [False, True])
def test_adc_dist_equals_the_oracle(ops, oracle, M, Ks, cb, nonfinite):
    rs = np.random.RandomState(M + Ks + cb)
    t = _table(rs, M, Ks, nonfinite)
    for N in (1, 257):
        c = _codes(rs, N, M, Ks, cb)
        with np.errstate(invalid='ignore'):
            want = oracle.dist_pqcodes_to_codebooks_c(t, c)
            assert np.array_equal(want, oracle.dist_pqcodes_to_codebooks_numpy(t, c), equal_nan=True)
        got = ops.adc_dist(ops.to_dev(t), ops.to_dev(c)).cpu().numpy()
        assert np.array_equal(got, want, equal_nan=True), (M, Ks, cb, N, nonfinite)


@on_gpu
@pytest.mark.parametrize('M,Ks,cb', [(3, 16, 1), (4, 16400, 2)])   # table in LDS / in global memory (4 * 16400 * 4 > 64 KiB)
def test_adc_dist_grid_stride_second_pass(ops, oracle, M, Ks, cb):
    """The grid is capped at 8 workgroups per CU: with more than 8 * CUs * 256 rows the stride loop runs a second pass (and a
    third for the first few rows of the third)."""
    import torch

    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cap = 8 * cus * 256
    N = 2 * cap + 300
    rs = np.random.RandomState(cus + M)
    t = _table(rs, M, Ks, True)
    c = _codes(rs, N, M, Ks, cb)
    with np.errstate(invalid='ignore'):
        want = oracle.dist_pqcodes_to_codebooks_c(t, c, threads=oracle.max_threads())
    got = ops.adc_dist(ops.to_dev(t), ops.to_dev(c)).cpu().numpy()
    bad = np.nonzero(~((got == want) | (np.isnan(got) & np.isnan(want))))[0]
    assert bad.size == 0, (N, cap, bad[:5])


@on_gpu
@pytest.mark.parametrize('M,Ks,cb', [(1, 256, 1), (3, 100, 1), (16, 256, 1), (128, 256, 1), (16, 512, 2), (3, 300, 4)])
@pytest.mark.parametrize('R', [1, 7, 64])
def test_adc_gather_equals_the_oracle(ops, oracle, M, Ks, cb, R):
    rs = np.random.RandomState(M + Ks + cb + R)
    N = 500
    c = _codes(rs, N, M, Ks, cb)
    for B in (1, 5):
        lut = np.stack([_table(rs, M, Ks, b % 2 == 1) for b in range(B)])
        cand = rs.randint(0, N, size=(B, R)).astype(np.int64)
        cand[rs.rand(B, R) < 0.15] = -1
        cand[rs.rand(B, R) < 0.1] = N                  # the first row beyond the table: +inf by definition
        cand[rs.rand(B, R) < 0.05] = N + (1 << 33)
        cand[:, R // 2:] = np.where(rs.rand(B, R - R // 2) < 0.5, cand[:, :1], cand[:, R // 2:])  # repeated candidates
        cand[0, 0], cand[-1, -1] = N - 1, 0               # the table's last row and its first
        want = np.full((B, R), np.inf, np.float32)
        with np.errstate(invalid='ignore'):
            for b in range(B):
                ok = (cand[b] >= 0) & (cand[b] < N)
                if cb == 1:
                    want[b] = oracle.adc_gather_c(lut[b], c, np.where(ok, cand[b], -1))
                elif ok.any():
                    want[b, ok] = oracle.dist_pqcodes_to_codebooks_c(lut[b], np.ascontiguousarray(c[cand[b][ok]]))
        got = ops.adc_gather(ops.to_dev(lut), ops.to_dev(c), ops.to_dev(cand)).cpu().numpy()
        assert np.array_equal(got, want, equal_nan=True), (M, Ks, cb, R, B)


# ------------------------------------------------------------------------------------------- GPU: codes_skew
SENTINEL = 0xA5


def _skew(ops, src, n, M, out, ids=None, id_base=0, inverse=False):
    """annlite_codes_skew with every extent spelled out: n rows move; the table side (``out`` forward, ``src`` inverse) must
    hold row max(id) = id_base + n - 1 or max(ids), the PLAIN side n rows."""
    from annlite_amd import _capi

    table, rows = (src, out) if inverse else (out, src)
    assert rows.shape[0] >= n and rows.shape[1] == M
    top = int(ids.max().item()) if ids is not None else id_base + n - 1
    assert table.shape[1] == M and table.shape[0] > top and (ids is None or (ids.numel() == n and int(ids.min().item()) >= 0))
    assert src.element_size() == out.element_size() == 1 and src.is_contiguous() and out.is_contiguous()
    _capi.check(_capi.lib().annlite_codes_skew(src.data_ptr(), n, M, None if ids is None else ids.data_ptr(), id_base, out.data_ptr(),
                                               int(inverse), _capi.stream_ptr()), 'codes_skew')


@on_gpu
@pytest.mark.parametrize('M', [1, 3, 8, 16, 32, 64, 128])
def test_codes_skew_forward_inverse_and_round_trip(ops, M):
    import torch

    rs = np.random.RandomState(M)
    n = 331
    plain = _wrap_rows(rs, n, M)
    pd_ = ops.to_dev(plain)
    # rows i -> table rows id_base + i
    for id_base in (0, 37):  # (37: not a multiple of any M here but 1)
        want = skew_rows(plain, id_base + np.arange(n))
        table = torch.full((id_base + n, M), SENTINEL, dtype=torch.uint8, device=pd_.device)
        _skew(ops, pd_, n, M, table, id_base=id_base)
        th = table.cpu().numpy()
        assert np.array_equal(th[id_base:], want), (M, id_base, np.argwhere(th[id_base:] != want)[:3])
        assert (th[:id_base] == SENTINEL).all()
        back = torch.full((n, M), SENTINEL, dtype=torch.uint8, device=pd_.device)
        _skew(ops, table, n, M, back, id_base=id_base, inverse=True)
        assert np.array_equal(back.cpu().numpy(), plain), (M, id_base)
        # the inverse of rows the REFERENCE stored (not the kernel's own output)
        stored = np.full((id_base + n, M), SENTINEL, np.uint8)
        stored[id_base:] = want
        back = torch.full((n, M), SENTINEL, dtype=torch.uint8, device=pd_.device)
        _skew(ops, ops.to_dev(stored), n, M, back, id_base=id_base, inverse=True)
        assert np.array_equal(back.cpu().numpy(), plain), (M, id_base)
    # scatter by ids into a larger table: untouched rows keep their bytes
    T = 3 * n + 5
    special = [31, 32, 63, 64]
    ids = np.array(special + [int(v) for v in rs.permutation(T) if v not in special][:n - 4], dtype=np.int64)
    assert len(set(ids.tolist())) == n and ids.max() < T
    table = torch.full((T, M), SENTINEL, dtype=torch.uint8, device=pd_.device)
    _skew(ops, pd_, n, M, table, ids=ops.to_dev(ids))
    want = np.full((T, M), SENTINEL, np.uint8)
    want[ids] = skew_rows(plain, ids)
    assert np.array_equal(table.cpu().numpy(), want), M
    sub = rs.permutation(n)[:100]
    back = torch.full((100, M), SENTINEL, dtype=torch.uint8, device=pd_.device)
    _skew(ops, table, 100, M, back, ids=ops.to_dev(ids[sub]), inverse=True)   # gather rows ids -> i
    assert np.array_equal(back.cpu().numpy(), plain[sub]), M


# ------------------------------------------------------------------------------------------- GPU: pq_search_seed_union
def _bound_keys(d):
    """The seed key of a row at distance d (scan_prep.hip: seed_bound_kernel): ``(key(d) + 2) << 32`` admits every row whose key is
    at most key(d) + 1, whatever its id -- the tightest bound a rank may publish for that row (the kernel's own add a rounding slack)."""
    return (f32_key(d) + np.uint64(2)) << np.uint64(32)


@on_gpu
def test_seed_union_bound_keeps_every_row_of_the_oracles_top_k(ops, oracle):
    """annlite_pq_search_split PREPARE -> annlite_pq_search_seed_union -> SCAN equals the oracle's top-k, with key sets that are
    valid by the header's contract and as TIGHT as it allows: the G ranks are disjoint row ranges that partition the table, each
    publishes the bounds of its true k smallest rows (oracle distances), so the k-th smallest of the union is exactly the bound
    of the table's k-th row -- a union that came out one rank too low would lose that row, and the comparison sees it.
    (a) G = 1, 2, 8 full key sets; (b) rows 300000.. repeat the codes of rows 0..: for the queries that sit on them two ranks
    publish the SAME key for two different rows, both counted; (c) ranks that publish fewer than k keys (all-ones entries) or
    none; (d) k = 1, 10, 16.  The rank's own seed bound is already in the prepared batch: the union only adds the peers' keys."""
    import torch
    from annlite_amd import _capi
    from annlite_amd._capi import LUT_L2, PHASE_PREPARE, PHASE_SCAN, SEED_KEYS

    rs = np.random.RandomState(11)
    N, M, dsub, Ks, B = 600_000, 16, 8, 256, 70
    D = M * dsub
    cb = rs.randn(M, Ks, dsub).astype(np.float32)
    A = rs.randn(8, D).astype(np.float32)
    cb_d = ops.to_dev(cb)
    codes_d = torch.empty((N, M), dtype=torch.uint8, device='cuda')
    x0 = None
    for c0 in range(0, N, 100_000):
        x = (rs.randn(100_000, 8).astype(np.float32) @ A + 0.05 * rs.randn(100_000, D).astype(np.float32)).astype(np.float32)
        x0 = x[:20].copy() if x0 is None else x0
        codes_d[c0:c0 + 100_000] = ops.pq_encode(ops.to_dev(x), cb_d)
    codes_d[300_000:301_000] = codes_d[0:1000]  # (b) the same code rows in two ranks of every split below with G > 1
    q = (rs.randn(B, 8).astype(np.float32) @ A + 0.05 * rs.randn(B, D).astype(np.float32)).astype(np.float32)
    q[:20] = x0                                 # ... and queries whose nearest rows are among them
    q_d = ops.to_dev(q)
    codes = codes_d.cpu().numpy()
    lut = oracle.batch_precompute_adc_table_c(q, dsub, Ks, cb)
    dist = np.stack([oracle.dist_pqcodes_to_codebooks_c(lut[b], codes, threads=oracle.max_threads()) for b in range(B)])
    cd = ops.codes_skew(codes_d)
    ws, state = ops.ScanWorkspace(), _capi.ScanState()
    ones = np.uint64(2 ** 64 - 1)
    seen_equal_keys = False
    for k in (10, 1, 16):
        want = [oracle.top_k_c(dist[b], k) for b in range(B)]
        rd, ri = np.stack([w[0] for w in want]), np.stack([w[1] for w in want])
        call = lambda phase, **kw: ops.pq_search_split(phase, LUT_L2, q_d, cb_d, cd, k, M, Ks, state, ws, codes_layout=1, **kw)
        own = None
        for _ in range(12):  # a few plain calls settle the kernel choice
            d, i = ops.pq_search_topk(LUT_L2, q_d, cb_d, cd, k, M, Ks, codes_layout=1, workspace=ws, state=state)
            torch.cuda.synchronize()
            assert np.array_equal(i.cpu().numpy(), ri) and np.array_equal(d.cpu().numpy(), rd)
            own = call(PHASE_PREPARE, seed_rows=4096)
            if own is not None:
                break
        assert own is not None, 'the state never settled on the byte-table kernel'
        for G in (1, 2, 8):
            edges = np.linspace(0, N, G + 1).astype(np.int64)
            full = np.full((G, B, SEED_KEYS), ones, np.uint64)
            for g in range(G):
                seg = dist[:, edges[g]:edges[g + 1]]
                full[g, :, :k] = _bound_keys(np.sort(np.partition(seg, k - 1, axis=1)[:, :k], axis=1))
            assert (np.diff(full[:, :, :k].astype(np.float64), axis=2) >= 0).all()
            if G > 1:
                seen_equal_keys |= bool((full[0, :20, 0] == full[G // 2, :20, 0]).any())
            short = full.copy()                                   # (c)
            short[1::2, :, k // 2:] = ones                        # every other rank: its k // 2 smallest rows only
            short[G - 1, :, :] = ones if G > 1 else short[G - 1]  # the last rank: nothing
            for name, keys in (('full', full), ('short', short)):
                assert call(PHASE_PREPARE, seed_rows=4096) is not None
                ops.pq_search_seed_union(ops.to_dev(keys), cd, B, k, M, Ks, ws)
                packed = call(PHASE_SCAN)
                torch.cuda.synchronize()
                p = packed.cpu().numpy()
                gi, gd = p[..., 0], (p[..., 1] & 0xFFFFFFFF).astype(np.uint32).view(np.float32)
                bad = np.nonzero((gi != ri).any(1))[0]
                assert bad.size == 0, (k, G, name, bad[:5], gi[bad[:1]], ri[bad[:1]])
                assert np.array_equal(gd, rd), (k, G, name)
    assert seen_equal_keys
