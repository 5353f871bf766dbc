"""CPU side of the float HNSW graph: the facade builds ``HnswFlatGpuIndex`` for ``graph=True, build='gpu'``
without ``n_subvectors`` -- constructing it needs no GPU -- and keeps refusing what does not exist over floats."""
import numpy as np
import pytest


def test_facade_with_graph_over_floats_builds_the_float_graph_index(tmp_path):
    from annlite_amd import AnnLite, HnswFlatGpuIndex, Metric
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex

    ann = AnnLite(64, graph=True, build='gpu', ef_search=77, max_connection=8, data_path=tmp_path / 'a')
    ix = ann.vec_index(0)
    assert type(ix) is HnswFlatGpuIndex and isinstance(ix, FlatGpuIndex)
    assert (ix.ef_search, ix.max_connection, ix.ef_construction, ix.build) == (77, 8, 200, 'gpu')
    assert ix.dim == 64 and ix.metric == Metric.COSINE and ix.size == 0 and ix.capacity == 10240
    assert ix.FORMAT != FlatGpuIndex.FORMAT
    assert ann.is_trained and ann.stat['is_trained'] is True
    ann2 = AnnLite(32, metric='euclidean', graph=True, build='gpu', ef_construction=40, data_path=tmp_path / 'a2')
    assert ann2.vec_index(0).ef_construction == 40 and ann2.vec_index(0).metric == Metric.EUCLIDEAN


def test_what_does_not_exist_over_floats_is_refused(tmp_path):
    from annlite_amd import AnnLite, HnswFlatGpuIndex

    with pytest.raises(NotImplementedError, match=r"graph.*build='gpu'"):  # no host library builds a float graph: an explicit opt-in
        AnnLite(64, graph=True, data_path=tmp_path / 'b')
    with pytest.raises(NotImplementedError, match='graph'):
        AnnLite(64, graph=True, build='host', data_path=tmp_path / 'c')
    with pytest.raises(NotImplementedError, match='graph'):
        AnnLite(64, graph=True, build='gpu', n_cells=4, ivf_prune=True, data_path=tmp_path / 'd')
    with pytest.raises(NotImplementedError, match='graph'):
        HnswFlatGpuIndex(64, build='host')
    with pytest.raises(ValueError, match='max_connection'):
        HnswFlatGpuIndex(64, max_connection=17)
    with pytest.raises(ValueError, match='2048'):
        HnswFlatGpuIndex(4096)


def test_rows_of_the_float_graph_are_not_updated_in_place():
    from annlite_amd import HnswFlatGpuIndex

    ix = HnswFlatGpuIndex(16)
    with pytest.raises(RuntimeError, match='in-place'):
        ix.update_with_ids(np.zeros((1, 16), np.float32), [0])
