"""CPU: the slack of ``annlite_vq_assign`` against explicit f32 ``fmaf`` chains, and the ``assign`` switch."""
import ctypes
import ctypes.util

import numpy as np
import pytest

F = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3


def _chain(a, b):
    """a j-ascending f32 ``fmaf`` chain of a[j] * b[j]: the MFMA's sum, and the selection kernel's with a = b = c - x"""
    acc = F(0)
    for j in range(len(a)):
        acc = F(_libm.fmaf(float(a[j]), float(b[j]), float(acc)))
    return acc


def _pairs(D, rs):
    x = rs.randn(4, D).astype(F)
    yield 'normal', x, rs.randn(4, D).astype(F)
    yield 'cancelling', x, (x * F(1 + 2 ** -20) + F(1e-6) * rs.randn(4, D)).astype(F)
    yield 'identical', x, x.copy()
    off = (1000.0 + 0.01 * rs.randn(8, D)).astype(F)
    yield 'offset', off[:4], off[4:]
    scale = (10.0 ** rs.uniform(-6, 6, size=(4, D))).astype(F)
    yield 'mixed magnitudes', (rs.randn(4, D) * scale).astype(F), (rs.randn(4, D) * scale[::-1]).astype(F)


@pytest.mark.parametrize('D', [1, 3, 33, 130, 768])
def test_slack_covers_the_score_against_the_chain(D):
    from annlite_amd import ops
    from annlite_amd.core.codec.vq import vq_assign_slack, vq_assign_slack_constants

    c_rel, c_abs = vq_assign_slack_constants(D)
    assert (c_rel, c_abs) == ops.vq_assign_slack(D)  # what the library launches the kernel with
    assert c_rel == F(1.05 * 2.0 ** -24 * (3.0 * D + (D + 63) // 64 + 24.0)) and c_abs == F(1e-30)
    worst = 0.0
    for name, xs, cs in _pairs(D, np.random.RandomState(D)):
        for x, c in zip(xs, cs):
            xn, cn = _chain(x, x), _chain(c, c)  # (any f32 order: the bound allows the kernels' shorter chains)
            s = F(cn - F(F(2) * _chain(c, x)))
            t = (c - x).astype(F)
            chain = _chain(t, t)
            eps = vq_assign_slack(D, xn, cn)
            assert eps.dtype == F
            x2 = float(np.dot(x.astype(np.float64), x.astype(np.float64)))
            err = abs(float(s) + x2 - float(chain))
            assert err <= float(eps), (name, D, err, eps)
            # ... and against float64: the chain itself is within the same bound of the real distance
            d64 = float(((c.astype(np.float64) - x.astype(np.float64)) ** 2).sum())
            assert abs(float(s) + x2 - d64) <= float(eps), (name, D)
            worst = max(worst, err / float(eps))
    assert D == 1 or worst > 0.0  # (the chains do differ: the check is not vacuous)


def test_assign_switch_and_old_pickles(tmp_path):
    from annlite_amd import AnnLite
    from annlite_amd.core.codec.vq import VQCodec

    codec = VQCodec(8)
    assert codec.assign == 'chain' and codec.last_assign_undecided == 0
    codec.assign = 'mfma'
    assert codec.assign == 'mfma' and hash(codec) == hash(VQCodec(8))
    with pytest.raises(ValueError, match='assign'):
        codec.assign = 'fast'
    state = codec.__getstate__()
    assert '_assign_ws' not in state
    del state['_assign_path']  # a file written before there was a choice
    old = VQCodec.__new__(VQCodec)
    old.__setstate__(state)
    assert old.assign == 'chain'

    ann = AnnLite(16, n_cells=4, n_subvectors=4, vq_assign='mfma', data_path=tmp_path / 'a')
    assert ann._vq_codec.assign == 'mfma'
    assert AnnLite(16, n_cells=4, n_subvectors=4, data_path=tmp_path / 'b')._vq_codec.assign == 'chain'
    assert AnnLite(16, vq_assign='mfma', data_path=tmp_path / 'c')._vq_codec is None  # ignored without a cell codec
    with pytest.raises(ValueError, match='vq_assign'):
        AnnLite(16, n_cells=4, n_subvectors=4, vq_assign='fast', data_path=tmp_path / 'd')
