"""CPU side of the split-bf16 filter over cell tiles ("split filter over cell tiles"): the ``cell_filter`` keyword
on ``IvfFlatGpuIndex`` and the facade (no GPU: storage is allocated on first use), and the offset layout's two filters restated in
numpy with their own constants."""
import numpy as np
import pytest

F = np.float32


def _vq(C):
    from annlite_amd.core.codec.vq import VQCodec

    return VQCodec(C)


def test_cell_filter_keyword_on_the_cell_index():
    from annlite_amd import ops
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex
    from annlite_amd.enums import Metric

    plain = IvfFlatGpuIndex(8, vq_codec=_vq(4))
    assert plain.cell_filter == 'f32' and plain.flat_filter == 'f32' and plain.last_cell_filter is None and plain.cell_centres_ is None
    assert plain._columns()['_cell_cnorms'] is None and plain._cell_cnorms is None
    stages = ops.ivf_flat_stages(150_000)
    new = IvfFlatGpuIndex(8, vq_codec=_vq(4), cell_filter='bf16x3')
    assert new.cell_filter == 'bf16x3' and new.flat_filter == 'f32' and new.last_cell_filter is None and new.cell_centres_ is None
    assert ops.ivf_flat_stages(150_000) == stages and len(stages) >= 3  # (the stages do not depend on the filter)
    # the centred-norms column exists for EUCLIDEAN only: the other metrics run the split filter on the values themselves
    assert new._columns()['_cell_cnorms'] is None  # (COSINE, the default metric)
    assert IvfFlatGpuIndex(8, vq_codec=_vq(4), metric=Metric.INNER_PRODUCT, cell_filter='bf16x3')._columns()['_cell_cnorms'] is None
    assert IvfFlatGpuIndex(8, vq_codec=_vq(4), metric=Metric.EUCLIDEAN, cell_filter='bf16x3')._columns()['_cell_cnorms'] is not None
    assert IvfFlatGpuIndex(8, vq_codec=_vq(4), metric=Metric.EUCLIDEAN)._columns()['_cell_cnorms'] is None
    # flat_filter / centre keep their treatment: popped and ignored
    both = IvfFlatGpuIndex(8, vq_codec=_vq(4), cell_filter='bf16x3', flat_filter='bf16x3', centre=None)
    assert both.cell_filter == 'bf16x3' and both.flat_filter == 'f32'
    for bad in ('fp8', 'bf16', None, 'f16x2'):
        with pytest.raises(ValueError, match="'f32'.*'bf16x3'"):
            IvfFlatGpuIndex(8, vq_codec=_vq(4), cell_filter=bad)
    with pytest.raises(ValueError, match='32768'):
        IvfFlatGpuIndex(32769, vq_codec=_vq(4), cell_filter='bf16x3')
    assert IvfFlatGpuIndex(32769, vq_codec=_vq(4)).cell_filter == 'f32'
    assert IvfFlatGpuIndex(32768, vq_codec=_vq(4), cell_filter='bf16x3').cell_filter == 'bf16x3'


def test_facade_forwards_cell_filter_to_the_cell_index_only(tmp_path):
    from annlite_amd import AnnLite
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.core.index.hnsw_flat_gpu import HnswFlatGpuIndex
    from annlite_amd.core.index.hnsw_pq_gpu import HnswPQGpuIndex
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex
    from annlite_amd.core.index.ivf_pq_gpu import IvfPQGpuIndex
    from annlite_amd.core.index.pq_flat_gpu import PQFlatGpuIndex

    cells = AnnLite(16, metric='euclidean', data_path=tmp_path / 'a', n_cells=4, n_probe=2, ivf_prune=True, cell_filter='bf16x3').vec_index(0)
    assert type(cells) is IvfFlatGpuIndex and cells.cell_filter == 'bf16x3' and cells.flat_filter == 'f32' and cells.n_probe == 2
    assert AnnLite(16, data_path=tmp_path / 'b', n_cells=4, ivf_prune=True).vec_index(0).cell_filter == 'f32'
    with pytest.raises(ValueError, match='cell_filter'):
        AnnLite(16, data_path=tmp_path / 'c', n_cells=4, ivf_prune=True, cell_filter='fp8')
    flat = AnnLite(16, data_path=tmp_path / 'd', cell_filter='bf16x3').vec_index(0)
    assert type(flat) is FlatGpuIndex and not hasattr(flat, 'cell_filter')
    graph = AnnLite(16, data_path=tmp_path / 'e', graph=True, build='gpu', cell_filter='bf16x3').vec_index(0)
    assert type(graph) is HnswFlatGpuIndex and not hasattr(graph, 'cell_filter')
    pq = AnnLite(16, data_path=tmp_path / 'f', n_subvectors=4, cell_filter='bf16x3').vec_index(0)
    assert type(pq) is PQFlatGpuIndex and not hasattr(pq, 'cell_filter')
    pq_cells = AnnLite(16, data_path=tmp_path / 'g', n_subvectors=4, n_cells=4, ivf_prune=True, cell_filter='bf16x3').vec_index(0)
    assert type(pq_cells) is IvfPQGpuIndex and not hasattr(pq_cells, 'cell_filter')
    pq_graph = AnnLite(16, data_path=tmp_path / 'h', n_subvectors=4, graph=True, cell_filter='bf16x3').vec_index(0)
    assert type(pq_graph) is HnswPQGpuIndex and not hasattr(pq_graph, 'cell_filter')


def test_offset_cells_pass_the_f32_comparison_and_not_the_centred_split_comparison():
    """The GPU test's offset layout (two cells of 5000 / 4500 rows around 1000 + the cube corners, D = 32, 50 queries, one probed cell,
    k = 10), both comparisons redone in float32 with the filters' own constants: the f32 filter passes every row of the probed cell
    (more than the list's 4096), the split filter centred on the cell's centroid a few dozen."""
    from annlite_amd import ops

    rs = np.random.RandomState(31)
    D, sizes, k = 32, [5000, 4500], 10
    cent = np.zeros((2, D), F)
    cent[:, 0] = [1.0, 7.0]
    cent = (cent + F(1000.0)).astype(F)
    cell = rs.permutation(np.repeat(np.arange(2), sizes))
    x = (cent[cell] + 0.3 * rs.randn(len(cell), D)).astype(F)
    qc = rs.randint(0, 2, size=50)
    q = (cent[qc] + 0.5 * rs.randn(50, D)).astype(F)
    cap = ops.flat_list_capacity()
    f_rel, f_abs = ops.flat_slack(1, D)
    s_rel, s_abs = ops.flat_split_slack(1, D)
    nx = (x * x).sum(1, dtype=F)
    passed_split = []
    for b in range(50):
        rows = np.flatnonzero(cell == qc[b])
        d = ((x[rows] - q[b]) ** 2).sum(1, dtype=F)
        thr = np.sort(d)[k - 1]
        a = (nx[rows] + (q[b] * q[b]).sum(dtype=F)).astype(F)
        v = (a - F(2) * (x[rows] @ q[b]).astype(F)).astype(F)
        n_f32 = int((~(v > thr + (f_rel * a + f_abs))).sum())
        assert n_f32 == len(rows) > cap, (b, n_f32)  # every row of the probed cell: the list overflows
        cx, cq = (x[rows] - cent[qc[b]]).astype(F), (q[b] - cent[qc[b]]).astype(F)
        a = ((cx * cx).sum(1, dtype=F) + (cq * cq).sum(dtype=F)).astype(F)
        v = (a - F(2) * (cx @ cq).astype(F)).astype(F)
        passed_split.append(int((~(v > thr + (s_rel * a + s_abs))).sum()))
    assert k <= min(passed_split) and max(passed_split) <= 64, passed_split  # (far below the list's 4096)
