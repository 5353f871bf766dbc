"""CPU side of the exact float32 search: the facade without ``n_subvectors``, the filter's slack restated
in numpy against f32 chains evaluated with libm's ``fmaf``, and the filter kernel's instructions."""
import ctypes
import ctypes.util
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'annlite_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
F = np.float32


def test_facade_without_n_subvectors_builds_the_float_index(tmp_path):
    from annlite_amd import AnnLite
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex

    ann = AnnLite(64, data_path=tmp_path / 'a')  # the reference's default configuration; needs no GPU to construct
    assert isinstance(ann.vec_index(0), FlatGpuIndex) and ann.vec_index(0).size == 0 and ann.vec_index(0).capacity == 10240
    assert ann.is_trained and ann.stat['is_trained'] is True and ann.stat['n_cells'] == 1 and ann.stat['index_size'] == 0
    ann.train(np.zeros((4, 64), np.float32))  # "not trainable": logs a warning and returns, index.py:206-210
    ann.train(np.zeros((4, 64), np.float32), force_train=True)
    assert ann.is_trained
    with pytest.raises(RuntimeError):
        ann.encode(np.zeros((1, 64), np.float32))
    d, i = ann.search_numpy(np.zeros((2, 64), np.float32))  # an empty index answers with empty lists
    assert len(d) == 2 and len(d[0]) == 0
    for kw in (dict(n_cells=4), dict(graph=True), dict(n_components=8)):
        with pytest.raises(NotImplementedError, match='n_cells|graph|n_components'):
            AnnLite(64, data_path=tmp_path / 'b', **kw)
    assert AnnLite(64, n_subvectors=8, data_path=tmp_path / 'c').is_trained is False  # the PQ path is what it was


# ---- the slack ------------------------------------------------------------------------------------------------------------------------
_libm = ctypes.CDLL(ctypes.util.find_library('m') or 'libm.so.6')
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3


def _fmaf(a, b, c):
    return F(_libm.fmaf(float(a), float(b), float(c)))


def _lane_chain(a, b):
    """rerank_topk_kernel's sum of a[j] * b[j]: 64 lane-strided fmaf chains, then the xor butterfly (f32 adds)."""
    s = np.zeros(64, F)
    for lane in range(64):
        acc = F(0)
        for j in range(lane, len(a), 64):
            acc = _fmaf(a[j], b[j], acc)
        s[lane] = acc
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[np.arange(64) ^ o]).astype(F)
    assert (s == s[0]).all() or np.isnan(s).all()
    return s[0]


def _k_chain(a, b):
    """The MFMA's sum: one k-ordered fmaf chain."""
    acc = F(0)
    for j in range(len(a)):
        acc = _fmaf(a[j], b[j], acc)
    return acc


def _pairs():
    rs = np.random.RandomState(3)
    for D in (3, 64, 128, 770):
        off = (1000.0 + 0.01 * rs.randn(12, D)).astype(F)  # a large common offset: |x|^2 - 2 q.x + |q|^2 cancels 8 digits
        yield 'offset', off[:6], off[6:]
        x = rs.randn(6, D).astype(F)
        yield 'near-duplicates', x, (x * F(1 + 2 ** -20) + F(1e-6) * rs.randn(6, D)).astype(F)
        yield 'identical', x, x.copy()
        scale = (10.0 ** rs.uniform(-6, 6, size=(6, D))).astype(F)
        yield 'mixed magnitudes', (rs.randn(6, D) * scale).astype(F), (rs.randn(6, D) * scale[::-1]).astype(F)
        yield 'tiny', (1e-18 * rs.randn(6, D)).astype(F), (1e-18 * rs.randn(6, D)).astype(F)


@pytest.mark.parametrize('metric', [1, 2])
def test_slack_covers_the_filter_chain_against_the_exact_chain(metric):
    from annlite_amd.core.index.flat_gpu import flat_slack_constants

    worst = 0.0
    for name, xs, qs in _pairs():
        D = xs.shape[1]
        c_rel, c_abs = flat_slack_constants(metric, D)  # what the library launches the filter kernel with
        assert c_rel.dtype == F and c_abs.dtype == F
        # ... and they are the constants DESIGN.md section 3.6 derives
        assert c_rel == F(1.05 * 2.0 ** -24 * (D + 3.0 * ((D + 63) // 64) + 40.0)) and c_abs == (F(1e-30) if metric == 1 else F(8 * 2.0 ** -24))
        for x, q in zip(xs, qs):
            a = F(_lane_chain(x, x) + _lane_chain(q, q))  # the two norms as flat_norms_kernel writes them
            dot = _k_chain(x, q)
            if metric == 1:
                t = (x - q).astype(F)
                exact = _lane_chain(t, t)
                v = F(a - F(F(2) * dot))
            else:
                exact = F(F(1) - _lane_chain(x, q))
                v = F(F(1) - dot)
            slack = F(F(c_rel * a) + c_abs)
            assert abs(float(v) - float(exact)) <= float(slack), (name, D, v, exact, slack)
            assert not (v > F(exact + slack)), (name, D)  # the kernel's own comparison, with the exact distance as the bound
            worst = max(worst, abs(float(v) - float(exact)) / float(slack))
    assert worst > 0.0  # (the chains do differ: the check is not vacuous)


# ---- the kernel's instructions --------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_filter_kernel_is_f32_mfma_without_scratch():
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, 'flat.s')
        cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S', '--cuda-device-only', 'flat.hip',
               '-o', asm]
        subprocess.run(cmd, cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        lines = open(asm).read().splitlines()
    starts = [(i, m.group(1)) for i, ln in enumerate(lines) for m in [re.match(r'^(_ZN7annlite18flat_filter_kernel\w+):', ln)] if m]
    assert len(starts) == 2, 'the two instantiations of flat_filter_kernel were not found in the assembly'
    for i0, sym in starts:
        i1 = next(j for j in range(i0, len(lines)) if lines[j].lstrip().startswith('.amdhsa_kernel ' + sym))
        body = lines[i0:i1]
        assert sum(re.search(r'\bv_mfma_f32_32x32x2_f32\b', ln) is not None for ln in body) >= 64, sym  # 16 depth steps x 2 x 2 tiles
        assert not any('scratch_' in ln for ln in body), (sym, 'scratch operations')
        assert not any(re.search(r'\bflat_(load|store|atomic)', ln) for ln in body), (sym, 'an LDS or global access lost its address space')
        head = '\n'.join(lines[i1:i1 + 80])
        assert re.search(r'\.amdhsa_private_segment_fixed_size 0\b', head), sym
