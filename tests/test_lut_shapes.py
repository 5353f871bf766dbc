"""``annlite_lut_build`` / ``annlite_lut_retile`` beyond the fixture shapes: L2 (VALU fmaf chain), IP and IPDIST (MFMA chain) in the
reference layout and the TILED layout, against the oracle's fp32 ``fmaf`` chains bit for bit (``view(np.uint32)``: -0 and +0
differ).  Shapes come from a pairwise selection over sub-vector width (the ragged MFMA tail at dsub 3, 5, 6, 7), code-book size
(Ks not a multiple of 16), batch (more than one 16-query tile) and sub-space count; plus subnormal operands and exact zeros.

Reference: pyx:85-274 (tables), pq.py:316-322 (IPDIST = float32(1 / Ks) - IP)."""
import itertools

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs an AMD GPU')]

DSUBS = [1, 2, 3, 5, 6, 7, 8, 12, 16, 32]
KSS = [1, 15, 16, 17, 100, 256, 700]
BS = [1, 15, 16, 17, 33, 257]
MS = [1, 3, 16, 64]


def _pairwise(*lists):
    """a greedy all-pairs cover: every value of every list meets every value of every other list in some row"""
    axes = list(itertools.combinations(range(len(lists)), 2))
    todo = {(i, a, j, b) for i, j in axes for a in range(len(lists[i])) for b in range(len(lists[j]))}
    rows = []
    while todo:
        best, gain = None, -1
        for cand in itertools.product(*[range(len(v)) for v in lists]):
            g = sum((i, cand[i], j, cand[j]) in todo for i, j in axes)
            if g > gain:
                best, gain = cand, g
        rows.append(tuple(lists[k][best[k]] for k in range(len(lists))))
        todo -= {(i, best[i], j, best[j]) for i, j in axes}
    return rows


CASES = _pairwise(DSUBS, KSS, BS, MS)


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _untile(flat, B, M, Ks, qi):
    """TILED [ceil(B16 / qi)][Ks][M][qi] (B16 = B padded to 16 queries) -> [B][M][Ks]; the pad queries are dropped"""
    Bp = (B + 15) // 16 * 16
    t = flat.reshape(Bp // qi, Ks, M, qi).transpose(0, 3, 2, 1).reshape(Bp, M, Ks)
    return t[:B]


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _check_all(ops, oracle, q, cb, what):
    from annlite_amd._capi import LAYOUT_BMK, LAYOUT_TILED, LUT_IP, LUT_IPDIST, LUT_L2

    B = q.shape[0]
    M, Ks, dsub = cb.shape
    th = oracle.max_threads()
    with np.errstate(all='ignore'):
        want = {LUT_L2: oracle.batch_precompute_adc_table_c(q, dsub, Ks, cb, threads=th),
                LUT_IP: oracle.batch_precompute_adc_table_ip_c(q, dsub, Ks, cb, threads=th),
                LUT_IPDIST: oracle.get_dist_mat_c(q, cb, oracle.INNER_PRODUCT, threads=th)}
    qd, cbd = ops.to_dev(q), ops.to_dev(cb)
    for kind, w in want.items():
        bmk = ops.lut_build(qd, cbd, kind, LAYOUT_BMK)
        assert _same_bits(bmk.cpu().numpy(), w), (what, kind, 'BMK')
        for qi in (2, 4):
            t = ops.lut_build(qd, cbd, kind, LAYOUT_TILED, qi).cpu().numpy()
            assert _same_bits(_untile(t, B, M, Ks, qi), w), (what, kind, 'TILED', qi)
        if kind == LUT_L2:
            for qi in (1, 2, 4):
                t = ops.lut_retile(bmk, qi).cpu().numpy()
                assert _same_bits(_untile(t, B, M, Ks, qi), w), (what, 'retile', qi)


@pytest.mark.parametrize('dsub,Ks,B,M', CASES, ids=lambda v: str(v))
def test_lut_shapes_equal_oracle(ops, oracle, dsub, Ks, B, M):
    while B * M * Ks > 3_000_000 and M > 1:  # (a few MB of table per case; the pair with B and Ks stays)
        M = {64: 16, 16: 3, 3: 1}[M]
    rs = np.random.RandomState(dsub * 7 + Ks * 11 + B * 13 + M)
    cb = rs.randn(M, Ks, dsub).astype(np.float32)
    q = rs.randn(B, M * dsub).astype(np.float32)
    _check_all(ops, oracle, q, cb, (dsub, Ks, B, M))


@pytest.mark.parametrize('dsub', [1, 3, 4, 7, 8])
def test_lut_subnormal_operands(ops, oracle, dsub):
    """products and partial sums in the subnormal range (and products that underflow to zero): the MFMA chain keeps them like the
    VALU chain (cdna_hip_programming.md section 3, 'FP32-input MFMA': C / D never flush, A / B follow the kernel's denorm mode)"""
    rs = np.random.RandomState(dsub)
    M, Ks, B = 4, 40, 19
    cb = (rs.randn(M, Ks, dsub) * 10.0 ** rs.randint(-22, -18, size=(M, Ks, dsub))).astype(np.float32)
    q = (rs.randn(B, M * dsub) * 10.0 ** rs.randint(-22, -18, size=(B, M * dsub))).astype(np.float32)
    q[0] = 1e-39          # subnormal operands themselves
    cb[:, 0] = -3e-40
    q[1] = 1e-30          # products far below the subnormal range: +-0
    tiny = np.finfo(np.float32).tiny
    with np.errstate(all='ignore'):
        ip = oracle.batch_precompute_adc_table_ip_c(q, dsub, Ks, cb)
        l2 = oracle.batch_precompute_adc_table_c(q, dsub, Ks, cb)
    sub = lambda t: ((t != 0) & (np.abs(t) < tiny)).sum()  # noqa: E731
    assert sub(ip) > 50 and sub(l2) > 50 and (ip == 0).any()
    _check_all(ops, oracle, q, cb, ('subnormal', dsub))


@pytest.mark.parametrize('dsub', [1, 2, 3, 5, 8])
def test_lut_orthogonal_pairs_and_signed_zeros(ops, oracle, dsub):
    """query / code word pairs with inner product exactly zero, -0 coordinates and code words equal to the query sub-vector: the
    zero entries must carry the oracle's sign"""
    rs = np.random.RandomState(40 + dsub)
    M, Ks, B = 3, 33, 18
    cb = rs.randint(-2, 3, size=(M, Ks, dsub)).astype(np.float32)
    q = rs.randint(-2, 3, size=(B, M * dsub)).astype(np.float32)
    cb[cb == 0] = -0.0
    q[::3][q[::3] == 0] = -0.0
    for m in range(M):
        qs = q[0, m * dsub:(m + 1) * dsub]
        cb[m, 1] = qs                          # L2 entry 0
        if dsub >= 2:
            cb[m, 2] = 0.0
            cb[m, 2, 0], cb[m, 2, 1] = -qs[1], qs[0]   # orthogonal to query 0's sub-vector
        cb[m, 3] = -0.0                        # -0 code word: products -0 or +0
    with np.errstate(all='ignore'):
        ip = oracle.batch_precompute_adc_table_ip_c(q, dsub, Ks, cb)
    assert (ip == 0).sum() > 5
    _check_all(ops, oracle, q, cb, ('zeros', dsub))
