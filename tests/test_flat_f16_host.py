"""CPU side of the half-precision row store of the exact float search ("f16 rows"): the f16 filter's slack
restated in numpy -- f16 by ``astype``, the power-of-two scale of the query, its two f16 planes, the two products summed in float64
and moved by the worst error the derivation allows the MFMA chain, f16 subnormal operands kept AND flushed, the norms and the exact
distance through libm's ``fmaf`` --, the keywords on the constructors and the facade, and the kernel's instructions."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from test_flat_host import _lane_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'annlite_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
F = np.float32
H = np.float16
U = 2.0 ** -24


def f16(a):
    """f32 -> the nearest f16 (ties to even; beyond 65504: inf), widened back: what the index stores, as the kernels read it."""
    with np.errstate(over='ignore'):
        return np.asarray(a, dtype=F).astype(H).astype(F)


def f16_constants(metric, D):
    """The formula DESIGN.md section 3.6 derives."""
    dp, nl = 16 * ((D + 15) // 16), (D + 63) // 64
    return F(1.05 * U * (4.4 * dp + 16.0 + 3.0 * nl + 44.0)), (F(2e-30) if metric == 1 else F(9 * U))


def query_scale(q):
    """e of flat_f16_queries_kernel: 14 - floor(log2 max |q_j|) clamped to [-126, 126]; 0 for an all-zero or non-finite query."""
    m = np.abs(q).max()
    if not np.isfinite(q).all() or m == 0:
        return 0
    return int(np.clip(15 - np.frexp(m)[1], -126, 126))


def query_planes(q):
    e = query_scale(q)
    qs = (q * F(2.0 ** e)).astype(F)
    qh = f16(qs)
    return e, qs, qh, f16((qs - qh).astype(F))


def flush(a):
    """an operand whose f16 subnormals the MFMA reads as zero"""
    return np.where(np.abs(a) < 2.0 ** -14, F(0), a).astype(F)


def _families():
    rs = np.random.RandomState(23)
    for D in (3, 64, 128, 770):
        x = rs.randn(6, D).astype(F)
        yield 'near-duplicates', x, (x * F(1 + 2 ** -20) + F(1e-6) * rs.randn(6, D)).astype(F)
        yield 'identical', x, f16(x)
        scale = (10.0 ** rs.uniform(-3, 3, size=(6, D))).astype(F)  # (inside the f16 range: |x| < 65504)
        yield 'mixed magnitudes', (rs.randn(6, D) * scale).astype(F), (rs.randn(6, D) * scale[::-1]).astype(F)
        yield 'tiny', (2e-6 * rs.randn(6, D)).astype(F), (1e-18 * rs.randn(6, D)).astype(F)  # rows: f16 subnormals (< 6.1e-5)
        yield 'tiny rows, unit queries', (2e-6 * rs.randn(6, D)).astype(F), rs.randn(6, D).astype(F)
        yield 'huge queries', rs.randn(6, D).astype(F), (1e30 * rs.randn(6, D)).astype(F)  # (|q|^2 overflows f32: everything passes)
        yield 'large queries', rs.randn(6, D).astype(F), (1e17 * rs.randn(6, D)).astype(F)
        m = F(1 + 2.0 ** -11 - 2.0 ** -23)  # just under an f16 tie in both halves of the QUERY split
        mk = lambda: (m * rs.choice([-1.0, 1.0], size=(6, D)) * 2.0 ** rs.randint(-3, 4, size=(6, D))).astype(F)
        yield 'adversarial mantissas', mk(), mk()


def test_f16_rounding_scale_and_planes():
    a = np.array([1.0, 1 + 2.0 ** -11, 1 + 2.0 ** -11 + 2.0 ** -23, 1 + 3 * 2.0 ** -11, 65504.0, 65519.9, 65520.0, -1e6, 3e-8, 2.0 ** -25], F)
    # ties to even; overflow; subnormals (3e-8 = 0.503 * 2^-24: the nearest is 2^-24; 2^-25 is a tie between 0 and 2^-24)
    want = np.array([1.0, 1.0, 1 + 2.0 ** -10, 1 + 2.0 ** -9, 65504.0, 65504.0, np.inf, -np.inf, 2.0 ** -24, 0.0], F)
    assert np.array_equal(f16(a), want)
    for q in (np.array([3.0, -0.1], F), np.array([1e-30, 0], F), np.array([-3e38, 1], F), np.array([1e-44, 0], F)):
        e, qs, qh, ql = query_planes(q)
        assert 2.0 ** 14 <= np.abs(qs).max() < 2.0 ** 15 or abs(e) == 126
        assert np.isfinite(qh).all() and np.isfinite(ql).all()  # a finite query never leaves the f16 range
        assert np.array_equal(qs.astype(np.float64), q.astype(np.float64) * 2.0 ** e) or e == -126  # (the scaling is exact)
        rho = np.abs(qs.astype(np.float64) - qh - ql)
        assert (rho <= 2.0 ** -22 * np.abs(qs) + 2.0 ** -14).all()
    assert query_scale(np.zeros(4, F)) == 0 and query_scale(np.array([1, np.nan], F)) == 0 and query_scale(np.array([np.inf, 1], F)) == 0
    assert query_scale(np.array([1.0], F)) == 14 and query_scale(np.array([1.99], F)) == 14 and query_scale(np.array([2.0], F)) == 13


@pytest.mark.parametrize('metric', [1, 2])
def test_f16_slack_covers_the_filter_value_against_the_exact_chain(metric):
    from annlite_amd.core.index.flat_gpu import flat_f16_slack_constants

    worst, seen = 0.0, 0
    for name, xs, qs in _families():
        D = xs.shape[1]
        c_rel, c_abs = flat_f16_slack_constants(metric, D)  # what the library launches the f16 filter with
        assert c_rel.dtype == F and c_abs.dtype == F
        assert (c_rel, c_abs) == f16_constants(metric, D)
        n_mfma = 2 * ((D + 15) // 16)
        chain = (1 + 34 * U) ** n_mfma - 1  # 17 truncating roundings (2u each) per MFMA, each over everything summed so far
        for x, q in zip(f16(xs), qs):  # (the rows as stored)
            e, _, qh, ql = query_planes(q)
            with np.errstate(over='ignore', invalid='ignore'):
                a = F(_lane_chain(x, x) + _lane_chain(q, q))  # the norms as the kernels write them, of the UNSCALED query
                if metric == 1:
                    t = (x - q).astype(F)
                    exact = _lane_chain(t, t)  # rerank_topk_kernel's distance on the widened row
                else:
                    exact = F(F(1) - _lane_chain(x, q))
                per_query = F(_lane_chain(np.abs(q), np.ones(D, F)) * F(1.001 * 2.0 ** -13))
                slack = F(F(F(c_rel * a) + c_abs) + per_query)
                for xo, ho, lo in ((x, qh, ql), (flush(x), flush(qh), flush(ql)), (flush(x), qh, ql), (x, flush(qh), flush(ql))):
                    terms = np.concatenate([xo.astype(np.float64) * ho, xo.astype(np.float64) * lo])
                    for acc in (F(terms.sum() - chain * np.abs(terms).sum()), F(terms.sum()), F(terms.sum() + chain * np.abs(terms).sum())):
                        dot = F(acc * F(2.0 ** -e))
                        v = F(a - F(F(2) * dot)) if metric == 1 else F(F(1) - dot)
                        assert not (v > F(exact + slack)), (name, D)  # the kernel's own comparison, with the exact distance as the bound
                        if np.isfinite(slack):
                            assert abs(float(v) - float(exact)) <= float(slack), (name, D, v, exact, slack)
                            worst = max(worst, abs(float(v) - float(exact)) / float(slack))
                            seen += 1
    assert 0.0 < worst <= 1.0 and seen > 1000  # (the values do differ: the check is not vacuous)


# ---- constructors and the facade (no GPU: storage is allocated on first use) --------------------------------------------------------
def test_dtype_keyword_on_the_float_indexes():
    import torch
    from annlite_amd.core.codec.vq import VQCodec
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.core.index.hnsw_flat_gpu import HnswFlatGpuIndex
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex
    from annlite_amd.enums import Metric

    for spelling in (np.float16, 'float16', 'half', np.dtype('float16')):
        idx = FlatGpuIndex(8, dtype=spelling)
        assert idx.flat_filter == 'f16x2' and idx.last_flat_filter is None and idx.centre_ is None
        assert idx._columns()['_vectors'] == ((8,), torch.float16) and idx._columns()['_cnorms'] is None
    assert FlatGpuIndex(8, dtype=np.float16, flat_filter='f16x2', metric=Metric.EUCLIDEAN).flat_filter == 'f16x2'
    for spelling in (np.float32, 'float32', 'float', np.float64):  # (every other dtype stores f32, as before)
        idx = FlatGpuIndex(8, dtype=spelling)
        assert idx.flat_filter == 'f32' and idx._columns()['_vectors'] == ((8,), torch.float32)
    assert FlatGpuIndex(8)._columns()['_vectors'] == ((8,), torch.float32)
    for bad in (dict(flat_filter='bf16x3'), dict(centre=None), dict(centre=np.zeros(8, F)), dict(flat_filter='bf16x3', centre=None)):
        with pytest.raises(ValueError, match='float16'):
            FlatGpuIndex(8, dtype=np.float16, metric=Metric.EUCLIDEAN, **bad)
    for kw in (dict(), dict(dtype=np.float32), dict(dtype='float64')):
        with pytest.raises(ValueError, match='f16x2'):
            FlatGpuIndex(8, flat_filter='f16x2', **kw)
    with pytest.raises(ValueError, match='32768'):
        FlatGpuIndex(32769, dtype=np.float16)
    with pytest.raises(NotImplementedError, match='float16'):
        HnswFlatGpuIndex(8, dtype=np.float16)
    with pytest.raises(NotImplementedError, match='float16'):
        HnswFlatGpuIndex(8, dtype='half', metric=Metric.EUCLIDEAN)
    with pytest.raises(NotImplementedError, match='float16'):
        IvfFlatGpuIndex(8, vq_codec=VQCodec(4), dtype=np.float16)
    assert HnswFlatGpuIndex(8, dtype=np.float32).flat_filter == 'f32'
    assert IvfFlatGpuIndex(8, vq_codec=VQCodec(4), dtype=np.float32).flat_filter == 'f32'


def test_facade_forwards_dtype_to_the_flat_index_only(tmp_path):
    from annlite_amd import AnnLite
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.core.index.pq_flat_gpu import PQFlatGpuIndex

    for n, spelling in enumerate((np.float16, 'float16')):
        flat = AnnLite(16, metric='euclidean', data_path=tmp_path / f'a{n}', dtype=spelling).vec_index(0)
        assert type(flat) is FlatGpuIndex and flat._f16 and flat.flat_filter == 'f16x2'
    assert not AnnLite(16, data_path=tmp_path / 'b').vec_index(0)._f16
    with pytest.raises(ValueError, match='float16'):
        AnnLite(16, data_path=tmp_path / 'c', dtype=np.float16, flat_filter='bf16x3')
    with pytest.raises(NotImplementedError, match='float16'):
        AnnLite(16, data_path=tmp_path / 'd', graph=True, build='gpu', dtype=np.float16)
    with pytest.raises(NotImplementedError, match='float16'):
        AnnLite(16, data_path=tmp_path / 'e', n_cells=4, ivf_prune=True, dtype=np.float16)
    pq = AnnLite(16, data_path=tmp_path / 'f', n_subvectors=4, dtype=np.float16).vec_index(0)  # (over PQ codes: ignored, as before)
    assert type(pq) is PQFlatGpuIndex
    AnnLite(16, data_path=tmp_path / 'g', n_subvectors=4, n_cells=4, dtype=np.float16)
    AnnLite(16, data_path=tmp_path / 'h', n_subvectors=4, graph=True, dtype=np.float16)


# ---- the kernel's instructions --------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_f16_filter_kernel_is_f16_mfma_without_scratch():
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, 'flat.s')
        cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S', '--cuda-device-only', 'flat.hip',
               '-o', asm]
        subprocess.run(cmd, cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        lines = open(asm).read().splitlines()
    starts = [(i, m.group(1)) for i, ln in enumerate(lines) for m in [re.match(r'^(_ZN7annlite22flat_f16_filter_kernel\w+):', ln)] if m]
    assert len(starts) == 2, 'the two instantiations of flat_f16_filter_kernel were not found in the assembly'
    for i0, sym in starts:
        i1 = next(j for j in range(i0, len(lines)) if lines[j].lstrip().startswith('.amdhsa_kernel ' + sym))
        body = lines[i0:i1]
        assert sum(re.search(r'\bv_mfma_f32_32x32x16_f16\b', ln) is not None for ln in body) >= 16, sym  # 2 K steps x 2 x (2 x 2) tiles
        assert not any('v_mfma_f32_32x32x16_bf16' in ln or 'v_mfma_f32_32x32x2_f32' in ln for ln in body), sym
        assert not any('scratch_' in ln for ln in body), (sym, 'scratch operations')
        assert not any(re.search(r'\bflat_(load|store|atomic)', ln) for ln in body), (sym, 'an LDS or global access lost its address space')
        head = '\n'.join(lines[i1:i1 + 80])
        assert re.search(r'\.amdhsa_private_segment_fixed_size 0\b', head), sym
