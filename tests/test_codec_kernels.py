"""The codec kernels (codec.hip) beyond the fixture shapes: encode (every templated sub-vector width, the generic kernel, the
LDS-overflow fallback, 1 / 2 / 4-byte codes, the grid-stride loop), decode, the k-means building blocks and l2_normalize.

Reference: encode / decode pq.py:158-198 (first minimum wins), fit pq.py:89-115 (Lloyd), l2_normalize math.py:6-18.  Encode and
the k-means counts run the oracle's fp32 ``fmaf`` chain (``pq_oracle.encode_c``): bit-exact.  Sums of fp32 atomics and the
normaliser's reduction are compared with float64 under the bounds stated at each check."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs an AMD GPU')]

EPS32 = 2.0 ** -24  # unit roundoff of float32


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _encode_u32(ops, xd, cbd):
    """annlite_pq_encode with code_bytes = 4 (ops.pq_encode only picks 4 bytes above 65536 code words)."""
    import torch

    from annlite_amd import _capi

    N, D = xd.shape
    M, Ks, _ = cbd.shape
    out = torch.full((N, M), -1, dtype=torch.int32, device=xd.device)
    _capi.check(_capi.lib().annlite_pq_encode(xd.data_ptr(), N, D, cbd.data_ptr(), M, Ks, out.data_ptr(), 4, _capi.stream_ptr()),
                'pq_encode')
    return out.cpu().numpy().view(np.uint32)


def _with_duplicates(rs, cb, x):
    """code words 2 and 5 (and Ks - 1 and 0) equal, rows sitting exactly on them: the first minimum must win"""
    M, Ks, dsub = cb.shape
    if Ks >= 6:
        cb[:, 5] = cb[:, 2]
        cb[:, Ks - 1] = cb[:, 0]
        for m in range(M):
            rows = rs.choice(x.shape[0], max(1, x.shape[0] // 8), replace=False)
            x[rows, m * dsub:(m + 1) * dsub] = cb[m, 2 if m % 2 else Ks - 1]
    return cb, x


def _encode_cases():
    dsubs = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16, 24, 32, 48]
    kss = [1, 2, 17, 100, 256, 257, 700]
    ns = [1, 255, 256, 257]
    out = []
    for i, dsub in enumerate(dsubs):
        for j in range(2):
            out.append((dsub, kss[(2 * i + j) % len(kss)], ns[(i + j) % len(ns)], 1 + (i + j) % 3))
    out.append((8, 4096, 257, 2))     # Ks * dsub * 4 = 128 KiB > 64 KiB: the templated width falls back to the generic kernel
    out.append((2, 256, 20000, 64))   # M = 64: the grid is capped at cu_count * 16 / M blocks -> the grid-stride loop
    return out


@pytest.mark.parametrize('dsub,Ks,N,M', _encode_cases(), ids=lambda v: str(v))
def test_encode_equals_oracle(ops, oracle, dsub, Ks, N, M):
    rs = np.random.RandomState(dsub * 1000 + Ks + N)
    cb = rs.randn(M, Ks, dsub).astype(np.float32)
    x = rs.randn(N, M * dsub).astype(np.float32)
    cb, x = _with_duplicates(rs, cb, x)
    want = oracle.encode_c(x, cb, threads=oracle.max_threads()).astype(np.uint32)
    if Ks >= 6:
        assert not np.isin(want, [5, Ks - 1]).any()  # (a later copy of a code word never wins)
    xd, cbd = ops.to_dev(x), ops.to_dev(cb)
    got = ops.codes_to_numpy(ops.pq_encode(xd, cbd))
    assert got.dtype == (np.uint8 if Ks <= 256 else np.uint16)
    assert np.array_equal(got.astype(np.uint32), want)
    assert np.array_equal(_encode_u32(ops, xd, cbd), want)


@pytest.mark.parametrize('dsub,Ks,code_dtype', [(1, 17, np.uint8), (3, 256, np.uint8), (7, 300, np.uint16), (48, 5, np.uint16),
                                                (5, 300, np.uint32), (2, 70000, np.uint32)])
def test_decode_equals_numpy_gather(ops, dsub, Ks, code_dtype):
    rs = np.random.RandomState(dsub + Ks)
    M, N = 3, 1001
    cb = rs.randn(M, Ks, dsub).astype(np.float32)
    codes = rs.randint(0, Ks, size=(N, M)).astype(code_dtype)
    codes[0] = Ks - 1
    codes[1] = 0
    want = np.concatenate([cb[m][codes[:, m].astype(np.int64)] for m in range(M)], axis=1)
    got = ops.pq_decode(ops.to_dev(codes), ops.to_dev(cb)).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------- k-means
def _kmeans_data(dsub, Ks, M, N, seed):
    rs = np.random.RandomState(seed)
    cb = rs.randn(M, Ks, dsub).astype(np.float32)
    x = (cb[np.arange(M)[None, :], rs.randint(0, Ks, size=(N, M))].reshape(N, M * dsub)
         + 0.3 * rs.randn(N, M * dsub)).astype(np.float32)
    cb[:, Ks - 1] = 50.0  # a centre no row is near: count 0
    return cb, x


def _accumulate(ops, xd, cbd, inertia=True, state=None):
    import torch

    M, Ks, dsub = cbd.shape
    if state is None:
        state = (torch.zeros((M, Ks, dsub), dtype=torch.float32, device=xd.device),
                 torch.zeros((M, Ks), dtype=torch.int32, device=xd.device),
                 torch.zeros((M,), dtype=torch.float64, device=xd.device) if inertia else None)
    ops.kmeans_assign_accumulate(xd, cbd, state[0], state[1], state[2])
    return state


def _reference_sums(oracle, x, cb):
    """float64 per-cluster sums, counts, sums of |x|, and the float64 total of the oracle's fp32 distances of the assigned centres"""
    M, Ks, dsub = cb.shape
    codes = oracle.encode_c(x, cb, threads=oracle.max_threads()).astype(np.int64)
    sums = np.zeros((M, Ks, dsub))
    abs_sums = np.zeros((M, Ks, dsub))
    counts = np.zeros((M, Ks), np.int64)
    inertia = np.zeros(M)
    for m in range(M):
        xm = x[:, m * dsub:(m + 1) * dsub].astype(np.float64)
        np.add.at(sums[m], codes[:, m], xm)
        np.add.at(abs_sums[m], codes[:, m], np.abs(xm))
        counts[m] = np.bincount(codes[:, m], minlength=Ks)
        d = oracle.cell_distances(x[:, m * dsub:(m + 1) * dsub], cb[m], 0)  # the same fp32 chain as the kernel's
        inertia[m] = d[np.arange(x.shape[0]), codes[:, m]].astype(np.float64).sum()
    return sums, abs_sums, counts, inertia


def _sum_bound(counts, abs_sums):
    """recursive fp32 summation in any order: |error| <= (n - 1) u sum|x_i| + O(u^2); stated as n * 2u * sum|x_i|"""
    return counts[..., None] * 2 * EPS32 * abs_sums


@pytest.mark.parametrize('dsub,Ks,M,N', [(4, 100, 3, 3000), (7, 50, 2, 2000), (1, 257, 2, 1500), (12, 16, 4, 777)],
                         ids=['templated', 'generic', 'dsub1_ks257', 'dsub12'])
def test_kmeans_assign_accumulate(ops, oracle, dsub, Ks, M, N):
    from annlite_amd import Metric, PQCodec

    cb, x = _kmeans_data(dsub, Ks, M, N, seed=dsub * 10 + Ks)
    ref_sums, abs_sums, ref_counts, ref_inertia = _reference_sums(oracle, x, cb)
    assert (ref_counts[:, Ks - 1] == 0).all()
    xd, cbd = ops.to_dev(x), ops.to_dev(cb)
    sums, counts, inertia = _accumulate(ops, xd, cbd)
    sums, counts, inertia = sums.cpu().numpy(), counts.cpu().numpy(), inertia.cpu().numpy()
    assert np.array_equal(counts, ref_counts)
    bound = _sum_bound(ref_counts, abs_sums)
    assert (np.abs(sums - ref_sums) <= bound).all(), np.max(np.abs(sums - ref_sums) - bound)
    np.testing.assert_allclose(inertia, ref_inertia, rtol=1e-6, atol=0)
    # a second call without zeroing adds to the first
    state = _accumulate(ops, xd, cbd)
    state = _accumulate(ops, xd, cbd, state=state)
    assert np.array_equal(state[1].cpu().numpy(), 2 * ref_counts)
    assert (np.abs(state[0].cpu().numpy() - 2 * ref_sums) <= 2 * _sum_bound(2 * ref_counts, abs_sums)).all()
    np.testing.assert_allclose(state[2].cpu().numpy(), 2 * ref_inertia, rtol=1e-6, atol=0)
    # no inertia buffer
    s_none, c_none, _ = _accumulate(ops, xd, cbd, inertia=False)
    assert np.array_equal(c_none.cpu().numpy(), ref_counts)
    assert (np.abs(s_none.cpu().numpy() - ref_sums) <= bound).all()
    # the deterministic host-ordered variant counts the same rows
    import torch

    codec = PQCodec(dim=M * dsub, n_subvectors=M, n_clusters=Ks, metric=Metric.EUCLIDEAN)
    det = (torch.zeros((M, Ks, dsub), dtype=torch.float32, device=xd.device), torch.zeros((M, Ks), dtype=torch.int32, device=xd.device),
           torch.zeros((M,), dtype=torch.float64, device=xd.device))
    codec._assign_accumulate_det(xd, cbd, *det)
    assert np.array_equal(det[1].cpu().numpy(), counts)


@pytest.mark.parametrize('dsub,Ks,M', [(1, 7, 2), (3, 100, 3), (8, 256, 2), (5, 33, 1)])
def test_kmeans_update_divides_and_keeps_empty_centres(ops, dsub, Ks, M):
    rs = np.random.RandomState(dsub * 100 + Ks)
    sums = (rs.randn(M, Ks, dsub) * 100).astype(np.float32)
    counts = rs.randint(0, 50, size=(M, Ks)).astype(np.int32)
    counts[:, ::5] = 0
    counts[0, 1] = 2 ** 24  # still exact as a float
    old = rs.randn(M, Ks, dsub).astype(np.float32)
    old[:, 0, 0] = -0.0
    old[:, 5, 0] = np.nan
    cbd = ops.to_dev(old)
    ops.kmeans_update(ops.to_dev(sums), ops.to_dev(counts), cbd)
    got = cbd.cpu().numpy()
    with np.errstate(all='ignore'):
        want = np.where(counts[..., None] > 0, sums / counts[..., None].astype(np.float32), old).astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    empty = counts == 0
    assert np.array_equal(got[empty].view(np.uint32), old[empty].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------- l2_normalize
THRESH = 10 * np.finfo(np.float32).eps  # math.py:14-16: rows with a norm below it are divided by 1


def _rel_bound(D):
    """relative error of x / sqrt(s) against float64: s sums ceil(D / 64) fma terms per lane and a 6-level butterfly (positive terms:
    relative error <= (ceil(D / 64) + 6) u), the square root halves it and adds u / 2, the division adds u / 2 (u = 2^-24).  The
    kernel's order can exceed 2 ulp of the result (2.15 ulp measured at D = 1000), so the bound is this one, not a fixed ulp count."""
    return ((-(-D // 64) + 6) / 2 + 1) * EPS32 * 1.01


@pytest.mark.parametrize('D', [1, 3, 63, 64, 65, 768, 1000])
def test_l2_normalize_against_float64(ops, D):
    import torch

    from annlite_amd import _capi

    rs = np.random.RandomState(D)
    N = 39  # not a multiple of the 4 rows of a workgroup
    x = rs.randn(N, D).astype(np.float32)
    x[1] *= 1e3
    x[2] *= 1e-3
    x[3] = 0.0
    x[4] = THRESH * (1 - 1e-3) / np.sqrt(D)  # norm just below the threshold: unchanged
    x[5] = THRESH * (1 + 1e-3) / np.sqrt(D)  # just above: normalised
    x[6] = 0.0
    x[6, D - 1] = -THRESH * 0.5
    x64 = x.astype(np.float64)
    norm = np.sqrt((x64 * x64).sum(1))
    below = norm < THRESH
    assert below[3] and below[4] and below[6] and not below[5]
    want = np.where(below[:, None], x64, x64 / np.where(below, 1.0, norm)[:, None])
    xd = ops.to_dev(x)
    got = ops.l2_normalize(xd).cpu().numpy()
    assert np.array_equal(got[below].view(np.uint32), x[below].view(np.uint32))
    nz = ~below[:, None] & (x != 0)
    err = np.abs(got.astype(np.float64) - want) / np.abs(np.where(nz, want, 1.0))
    assert (err[nz] <= _rel_bound(D)).all(), (err[nz].max(), _rel_bound(D))
    assert np.array_equal(got[x == 0], x[x == 0])
    # in place through the C entry (out is x): the same bits
    _capi.check(_capi.lib().annlite_l2_normalize(xd.data_ptr(), N, D, xd.data_ptr(), _capi.stream_ptr()), 'l2_normalize')
    torch.cuda.synchronize()
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), got.view(np.uint32))
