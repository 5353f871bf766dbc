"""CPU side of ``filter_route`` ("selected rows"): the keyword on the constructors, per call and through the
facade; the pure decision of ``'auto'`` at its edges; the indexes over PQ codes accept the keyword and drop it."""
import numpy as np
import pytest

F = np.float32


def test_the_keyword_on_the_float_indexes():
    from annlite_amd.core.codec.vq import VQCodec
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.core.index.hnsw_flat_gpu import HnswFlatGpuIndex
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex
    from annlite_amd.enums import Metric

    assert FlatGpuIndex.FILTER_ROUTES == ('mask', 'rows', 'auto')
    idx = FlatGpuIndex(8)
    assert idx.filter_route == 'mask' and idx.last_filter_route is None and idx._sel_rows is None
    for route in FlatGpuIndex.FILTER_ROUTES:
        for kw in (dict(), dict(dtype=np.float16), dict(dtype=np.int8), dict(flat_filter='bf16x3', metric=Metric.EUCLIDEAN)):
            assert FlatGpuIndex(8, filter_route=route, **kw).filter_route == route
        assert HnswFlatGpuIndex(8, filter_route=route).filter_route == route
        vq = VQCodec(4, metric=Metric.EUCLIDEAN)
        assert IvfFlatGpuIndex(8, vq_codec=vq, filter_route=route).filter_route == route
    for bad in ('Mask', 'row', '', None, 1, 'gpu'):
        with pytest.raises(ValueError, match='filter_route'):
            FlatGpuIndex(8, filter_route=bad)
        with pytest.raises(ValueError, match='filter_route'):
            HnswFlatGpuIndex(8, filter_route=bad)


def test_the_keyword_per_call_is_validated_before_anything_runs():
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex

    idx = FlatGpuIndex(8)
    for bad in ('bogus', 'ROWS', 3):
        with pytest.raises(ValueError, match='filter_route'):
            idx.choose_filter_route(10, 100, 10, route=bad)


def test_the_auto_decision_at_its_edges():
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex

    frac = FlatGpuIndex.ROWS_MAX_FRACTION
    assert 0 < frac <= 1
    n = 1_000_000
    at = int(frac * n)  # the largest selection that is at most the fraction of the rows
    assert at <= frac * n < at + 1
    auto, rows, mask = (FlatGpuIndex(8, filter_route=r) for r in ('auto', 'rows', 'mask'))
    # 'auto': by the share of the rows
    assert auto.choose_filter_route(0, n, 10) == 'rows'
    assert auto.choose_filter_route(1, n, 10) == 'rows'
    assert auto.choose_filter_route(at, n, 10) == 'rows'
    if at < n:
        assert auto.choose_filter_route(at + 1, n, 10) == 'mask'
        assert auto.choose_filter_route(n, n, 10) == 'mask'
    assert auto.choose_filter_route(at, n, 64) == 'rows'
    # limit > 64 keeps the masked search, and a search with nothing to compact stays what it was -- under every value
    for idx in (auto, rows, mask):
        assert idx.choose_filter_route(1, n, 65) == 'mask'
        assert idx.choose_filter_route(None, n, 10) == 'mask'
    # the two orders
    for n_sel in (0, 1, at, n):
        assert rows.choose_filter_route(n_sel, n, 10) == 'rows'
        assert mask.choose_filter_route(n_sel, n, 10) == 'mask'
    # the call's keyword goes before the index's
    assert mask.choose_filter_route(1, n, 10, route='rows') == 'rows'
    assert rows.choose_filter_route(1, n, 10, route='mask') == 'mask'
    assert mask.choose_filter_route(1, n, 10, route='auto') == 'rows'
    # an empty table: nothing is selected, nothing is above the fraction
    assert auto.choose_filter_route(0, 0, 10) == 'rows'


def test_the_indexes_over_pq_codes_accept_the_keyword_and_drop_it():
    from annlite_amd.core.codec.pq import PQCodec
    from annlite_amd.core.codec.vq import VQCodec
    from annlite_amd.core.index.hnsw_pq_gpu import HnswPQGpuIndex
    from annlite_amd.core.index.ivf_pq_gpu import IvfPQGpuIndex
    from annlite_amd.core.index.pq_flat_gpu import PQFlatGpuIndex
    from annlite_amd.enums import Metric

    pq = PQCodec(dim=8, n_subvectors=2, n_clusters=4).set_codebooks(np.zeros((2, 4, 4), F))
    for route in ('mask', 'rows', 'auto'):
        for idx in (PQFlatGpuIndex(dim=8, pq_codec=pq, metric=Metric.EUCLIDEAN, filter_route=route),
                    HnswPQGpuIndex(dim=8, pq_codec=pq, metric=Metric.EUCLIDEAN, filter_route=route),
                    IvfPQGpuIndex(dim=8, pq_codec=pq, vq_codec=VQCodec(4, metric=Metric.EUCLIDEAN), metric=Metric.EUCLIDEAN, filter_route=route)):
            assert not hasattr(idx, 'filter_route') and not hasattr(idx, 'last_filter_route')


def test_the_facade_hands_the_keyword_to_the_float_indexes_only(tmp_path):
    from annlite_amd import AnnLite
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.core.index.hnsw_flat_gpu import HnswFlatGpuIndex

    ann = AnnLite(16, columns=[('a', int)], filter_route='rows', data_path=tmp_path / 'a')
    assert type(ann.vec_index(0)) is FlatGpuIndex and ann.vec_index(0).filter_route == 'rows'
    assert AnnLite(16, data_path=tmp_path / 'b').vec_index(0).filter_route == 'mask'
    ann = AnnLite(16, graph=True, build='gpu', filter_route='auto', data_path=tmp_path / 'c')
    assert type(ann.vec_index(0)) is HnswFlatGpuIndex and ann.vec_index(0).filter_route == 'auto'
    with pytest.raises(ValueError, match='filter_route'):
        AnnLite(16, filter_route='bogus', data_path=tmp_path / 'd')
    pq = AnnLite(16, n_subvectors=4, filter_route='rows', data_path=tmp_path / 'e')  # (over PQ codes: dropped)
    assert not hasattr(pq.vec_index(0), 'filter_route')
