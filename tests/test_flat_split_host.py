"""CPU side of the split-bf16 filter of the exact float32 search ("split filter"): its slack restated in
numpy -- bf16 round-to-nearest-even by bit arithmetic, the three products summed in float64 and moved by the worst error the
derivation allows the MFMA chain, the centred norms and the exact distance through libm's ``fmaf`` --, the keywords on the
constructors and the facade, and the kernel's instructions."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from test_flat_host import _lane_chain, _pairs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'annlite_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
F = np.float32
U = 2.0 ** -24


def bf16_rne(a):
    """f32 -> the nearest bf16 (ties to even), as an f32 array: what v_cvt_pk_bf16_f32 does to a finite value."""
    bits = np.ascontiguousarray(a, dtype=F).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(F)


def split(c):
    h = bf16_rne(c)
    return h, bf16_rne((c - h).astype(F))


def split_constants(metric, D):
    """The formula DESIGN.md section 3.6 derives."""
    dp, nl = 16 * ((D + 15) // 16), (D + 63) // 64
    return F(1.05 * U * (6.6 * dp + 780.0 + 3.0 * nl + 44.0)), (F(2e-30) if metric == 1 else F(9 * U))


def _families():
    """test_flat_host's families, the offset one with and without its centre, and mantissas that sit just under a bf16 tie."""
    rs = np.random.RandomState(11)
    for name, xs, qs in _pairs():
        D = xs.shape[1]
        yield name, xs, qs, None
        if name == 'offset':
            yield 'offset, centred', xs, qs, np.full(D, 1000.0, F)
            yield 'offset, centred on the mean', xs, qs, np.concatenate([xs, qs]).mean(axis=0).astype(F)
    for D in (3, 64, 128, 770):
        m = F(1 + 2.0 ** -8 - 2.0 ** -20)
        mk = lambda: (m * rs.choice([-1.0, 1.0], size=(6, D)) * 2.0 ** rs.randint(-3, 4, size=(6, D))).astype(F)
        yield 'adversarial mantissas', mk(), mk(), None


def test_bf16_rounding_by_bits():
    a = np.array([1.0, 1 + 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8 - 2.0 ** -20), 3.4e38, 1e-40], F)
    want = np.array([1.0, 1.0, 1 + 2.0 ** -7, 1 + 2.0 ** -6, -1.0, np.inf, 1e-40], F)
    got = bf16_rne(a)
    assert np.array_equal(got[:6], want[:6]) and abs(float(got[6]) - 1e-40) <= 2.0 ** -134  # (ties to even; overflow; a subnormal)
    h, l = split(a[:5])
    assert (np.abs(a[:5].astype(np.float64) - h - l) <= 2.0 ** -16 * np.abs(a[:5])).all()


@pytest.mark.parametrize('metric', [1, 2])
def test_split_slack_covers_the_filter_value_against_the_exact_chain(metric):
    from annlite_amd.core.index.flat_gpu import flat_split_slack_constants

    worst = 0.0
    for name, xs, qs, mu in _families():
        if metric != 1 and mu is not None:
            continue  # (a centre is EUCLIDEAN's)
        D = xs.shape[1]
        c_rel, c_abs = flat_split_slack_constants(metric, D)  # what the library launches the split filter with
        assert c_rel.dtype == F and c_abs.dtype == F
        assert (c_rel, c_abs) == split_constants(metric, D)
        n_mfma = 3 * ((D + 15) // 16)
        chain = (1 + 34 * U) ** n_mfma - 1  # 17 truncating roundings (2u each) per MFMA, each over everything summed so far
        for x, q in zip(xs, qs):
            cx, cq = (x if mu is None else (x - mu).astype(F)), (q if mu is None else (q - mu).astype(F))
            (xh, xl), (qh, ql) = split(cx), split(cq)
            terms = np.concatenate([qh.astype(np.float64) * xh, qh.astype(np.float64) * xl, ql.astype(np.float64) * xh])
            a = F(_lane_chain(cx, cx) + _lane_chain(cq, cq))  # the centred norms as the kernels write them
            if metric == 1:
                t = (x - q).astype(F)
                exact = _lane_chain(t, t)  # rerank_topk_kernel's distance, on the UNCENTRED values
            else:
                exact = F(F(1) - _lane_chain(x, q))
            slack = F(F(c_rel * a) + c_abs)
            for dot in (F(terms.sum() - chain * np.abs(terms).sum()), F(terms.sum()), F(terms.sum() + chain * np.abs(terms).sum())):
                v = F(a - F(F(2) * dot)) if metric == 1 else F(F(1) - dot)
                assert abs(float(v) - float(exact)) <= float(slack), (name, D, v, exact, slack)
                assert not (v > F(exact + slack)), (name, D)  # the kernel's own comparison, with the exact distance as the bound
                worst = max(worst, abs(float(v) - float(exact)) / float(slack))
    assert 0.0 < worst <= 1.0  # (the values do differ: the check is not vacuous)


def test_offset_rows_pass_the_f32_slack_and_not_the_centred_split_slack():
    """The issue's probe: 1000 + N(0, 1), D = 32 -- the f32 slack exceeds every distance, the centred split slack almost none."""
    from annlite_amd.core.index.flat_gpu import flat_slack_constants, flat_split_slack_constants

    rs = np.random.RandomState(5)
    x = (1000.0 + rs.randn(2048, 32)).astype(F)
    q = (1000.0 + rs.randn(32)).astype(F)
    d = ((x.astype(np.float64) - q) ** 2).sum(1)
    bound = np.sort(d)[9]
    c_rel, c_abs = flat_slack_constants(1, 32)
    s_f32 = c_rel * ((x.astype(np.float64) ** 2).sum(1) + (q.astype(np.float64) ** 2).sum()) + c_abs
    mu = x.mean(axis=0).astype(F)
    c_rel, c_abs = flat_split_slack_constants(1, 32)
    s_split = c_rel * (((x - mu).astype(np.float64) ** 2).sum(1) + ((q - mu).astype(np.float64) ** 2).sum()) + c_abs
    assert (d <= bound + 2 * s_f32).all()              # every row is inside the f32 filter's reach
    assert (d <= bound + 2 * s_split).sum() <= 12      # the ten nearest and at most a tie or two


# ---- constructors and the facade (no GPU: storage is allocated on first use) --------------------------------------------------------
def test_keywords_on_the_float_indexes():
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.core.index.hnsw_flat_gpu import HnswFlatGpuIndex
    from annlite_amd.enums import Metric

    plain = FlatGpuIndex(8)
    assert plain.flat_filter == 'f32' and plain.centre_ is None and plain.last_flat_filter is None and plain._cnorms is None
    idx = FlatGpuIndex(8, metric=Metric.EUCLIDEAN, flat_filter='bf16x3')
    assert idx.flat_filter == 'bf16x3' and idx.centre == 'mean' and idx.centre_ is None and '_cnorms' in idx._columns()
    assert idx._columns()['_cnorms'] is not None
    for kw in (dict(metric=Metric.COSINE), dict(metric=Metric.INNER_PRODUCT), dict(metric=Metric.EUCLIDEAN, centre=None)):
        assert FlatGpuIndex(8, flat_filter='bf16x3', **kw)._columns()['_cnorms'] is None  # (no centre: no second norms column)
    given = FlatGpuIndex(3, metric=Metric.EUCLIDEAN, flat_filter='bf16x3', centre=[1, 2, 3])
    assert given.centre.dtype == F and given.centre.tolist() == [1.0, 2.0, 3.0]
    g = HnswFlatGpuIndex(8, metric=Metric.EUCLIDEAN, flat_filter='bf16x3', centre=None)
    assert g.flat_filter == 'bf16x3' and g.centre is None and g.filter_search == 'exact'
    for bad in (dict(flat_filter='bf16'), dict(flat_filter=None), dict(centre='median'), dict(centre=np.zeros(3, F)),
                dict(centre=np.zeros((1, 8), F))):
        for cls in (FlatGpuIndex, HnswFlatGpuIndex):
            with pytest.raises(ValueError, match='flat_filter|centre'):
                cls(8, **bad)
    with pytest.raises(ValueError, match='32768'):
        FlatGpuIndex(32769, flat_filter='bf16x3')
    assert FlatGpuIndex(32769).flat_filter == 'f32'


def test_facade_forwards_the_keywords_to_the_float_indexes_only(tmp_path):
    from annlite_amd import AnnLite
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.core.index.hnsw_flat_gpu import HnswFlatGpuIndex
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex
    from annlite_amd.core.index.pq_flat_gpu import PQFlatGpuIndex

    flat = AnnLite(16, metric='euclidean', data_path=tmp_path / 'a', flat_filter='bf16x3', centre=None).vec_index(0)
    assert type(flat) is FlatGpuIndex and flat.flat_filter == 'bf16x3' and flat.centre is None
    assert AnnLite(16, data_path=tmp_path / 'b').vec_index(0).flat_filter == 'f32'
    graph = AnnLite(16, metric='euclidean', data_path=tmp_path / 'c', graph=True, build='gpu', flat_filter='bf16x3').vec_index(0)
    assert type(graph) is HnswFlatGpuIndex and graph.flat_filter == 'bf16x3' and graph.centre == 'mean'
    with pytest.raises(ValueError, match='flat_filter'):
        AnnLite(16, data_path=tmp_path / 'd', flat_filter='fp8')
    cells = AnnLite(16, data_path=tmp_path / 'e', n_cells=4, ivf_prune=True, flat_filter='bf16x3', centre=None).vec_index(0)
    assert type(cells) is IvfFlatGpuIndex and cells.flat_filter == 'f32'  # (accepted and ignored: the cell tiles keep the f32 filter)
    pq = AnnLite(16, data_path=tmp_path / 'f', n_subvectors=4, flat_filter='bf16x3', centre=None).vec_index(0)
    assert type(pq) is PQFlatGpuIndex and not hasattr(pq, 'flat_filter')
    AnnLite(16, data_path=tmp_path / 'g', n_subvectors=4, graph=True, flat_filter='bf16x3')  # (dropped there as well)


# ---- the kernel's instructions --------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_split_filter_kernel_is_bf16_mfma_without_scratch():
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, 'flat.s')
        cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-S', '--cuda-device-only', 'flat.hip',
               '-o', asm]
        subprocess.run(cmd, cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        lines = open(asm).read().splitlines()
    starts = [(i, m.group(1)) for i, ln in enumerate(lines) for m in [re.match(r'^(_ZN7annlite24flat_split_filter_kernel\w+):', ln)] if m]
    assert len(starts) == 2, 'the two instantiations of flat_split_filter_kernel were not found in the assembly'
    for i0, sym in starts:
        i1 = next(j for j in range(i0, len(lines)) if lines[j].lstrip().startswith('.amdhsa_kernel ' + sym))
        body = lines[i0:i1]
        assert sum(re.search(r'\bv_mfma_f32_32x32x16_bf16\b', ln) is not None for ln in body) >= 24, sym  # 2 K steps x 3 x (2 x 2) tiles
        head = '\n'.join(lines[i1:i1 + 80])
        assert re.search(r'\.amdhsa_private_segment_fixed_size 0\b', head), sym
