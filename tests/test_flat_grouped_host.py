"""CPU side of a filter per query ("a filter per query"): the grouping of equal filters and its length check,
the split of more than ``MAX_FILTER_GROUPS`` groups into launches, and the argument checks and workspace sizes of the three C entries
through ``_capi`` (the library loads without a GPU: every check below fails before anything touches a device)."""
import ctypes

import numpy as np
import pytest


# ---- the grouping -------------------------------------------------------------------------------------------------------------------
def test_equal_filters_form_one_group_in_order_of_first_appearance():
    from annlite_amd.core.index.row_store import group_filters

    a, b = {'tenant': {'$eq': 1}}, {'x': {'$lt': 0.5}, 'tenant': 3}
    filters = [b, None, a, {'tenant': {'$eq': 1}}, {}, b, {'tenant': 3, 'x': {'$lt': 0.5}}, a]
    distinct, group_of = group_filters(filters, len(filters))
    assert distinct == [b, None, a]  # order kept; None and {} are one group, named None; dicts compare by ==, not by identity or key order
    assert group_of.dtype == np.int64 and group_of.tolist() == [0, 1, 2, 2, 1, 0, 0, 2]
    # a tuple is a list; all equal: one group
    distinct, group_of = group_filters((a, dict(a), a), 3)
    assert distinct == [a] and group_of.tolist() == [0, 0, 0]
    distinct, group_of = group_filters([{}, None], 2)
    assert distinct == [None] and group_of.tolist() == [0, 0]
    distinct, group_of = group_filters([], 0)
    assert distinct == [] and group_of.shape == (0,)
    # $eq 1 and $eq 1.0 are equal dicts, $eq 1 and $eq 2 are not
    assert len(group_filters([{'n': {'$eq': 1}}, {'n': {'$eq': 1.0}}, {'n': {'$eq': 2}}], 3)[0]) == 2


def test_the_length_and_the_entries_are_checked():
    from annlite_amd.core.index.row_store import group_filters

    for filters, n in (([None], 2), ([None, None, None], 2), ([], 1), (({},), 0)):
        with pytest.raises(ValueError, match='one filter per query'):
            group_filters(filters, n)
    with pytest.raises(ValueError, match='dict'):
        group_filters([None, 'tenant == 1'], 2)
    with pytest.raises(ValueError, match='dict'):
        group_filters([[{}]], 1)


def test_the_facade_checks_the_length_before_anything_runs(tmp_path):
    from annlite_amd import AnnLite

    ann = AnnLite(8, metric='euclidean', data_path=tmp_path, columns=[('tenant', int)])
    assert ann.last_filter_batch is None and ann.last_filter_groups is None
    q = np.zeros((3, 8), np.float32)
    for bad in ([None], [{}, {}], [None] * 4, ()):
        with pytest.raises(ValueError, match='one filter per query'):
            ann.search_numpy(q, filter=bad)
        with pytest.raises(ValueError, match='one filter per query'):
            ann.search_by_vectors(q, filter=bad)


def test_more_groups_than_a_launch_takes_are_split():
    from annlite_amd.core.index.row_store import RowStoreIndex, group_chunks

    assert RowStoreIndex.MAX_FILTER_GROUPS == 64
    # one launch: every query, the groups that HAVE queries renumbered densely
    group_of = np.array([5, 0, 5, 9, 0], dtype=np.int64)
    (groups, queries, local), = group_chunks(group_of, 64)
    assert groups.tolist() == [0, 5, 9] and queries is None and local.tolist() == [1, 0, 1, 2, 0]
    # 64 groups still fit, 65 do not
    assert len(group_chunks(np.arange(64), 64)) == 1
    rs = np.random.RandomState(3)
    group_of = rs.permutation(np.repeat(np.arange(150), 3))  # 150 groups of three queries
    chunks = group_chunks(group_of, 64)
    assert [len(c[0]) for c in chunks] == [64, 64, 22]
    seen = np.zeros(len(group_of), dtype=int)
    for groups, queries, local in chunks:
        assert (np.diff(queries) > 0).all() and local.min() >= 0 and local.max() < len(groups)
        assert np.array_equal(groups[local], group_of[queries])  # a query keeps its group under the launch's numbering
        seen[queries] += 1
    assert (seen == 1).all()  # every query in exactly one launch


def test_group_ids_are_checked_on_the_host():
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex

    idx = FlatGpuIndex(4)
    assert idx.last_filter_batch is None
    assert idx._check_groups(3, [None, None], [1, 0, 1]).tolist() == [1, 0, 1]
    for bad in ([0, 2, 0], [-1, 0, 0], [0, 0], [0, 0, 0, 0]):
        with pytest.raises(ValueError, match='group_of'):
            idx._check_groups(3, [None, None], bad)


def test_the_pruned_and_the_graph_index_keep_the_looping_form():
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.core.index.hnsw_flat_gpu import HnswFlatGpuIndex
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex
    from annlite_amd.core.index.pq_flat_gpu import PQFlatGpuIndex
    from annlite_amd.core.index.row_store import RowStoreIndex

    base = RowStoreIndex.search_batch_grouped
    assert FlatGpuIndex.search_batch_grouped is not base
    for cls in (HnswFlatGpuIndex, IvfFlatGpuIndex, PQFlatGpuIndex):
        assert cls.search_batch_grouped is base, cls


# ---- the C entries -------------------------------------------------------------------------------------------------------------------
def _lib():
    from annlite_amd import _capi

    return _capi, _capi.lib()


def test_the_workspace_is_the_filters_own():
    _capi, lib = _lib()
    grouped, need = ctypes.c_int64(0), ctypes.c_int64(0)
    own = {'f32': lambda *a: lib.annlite_flat_search_workspace_bytes(*a), 'bf16x3': lambda *a: lib.annlite_flat_search_split_workspace_bytes(*a),
           'f16x2': lambda *a: lib.annlite_flat_search_f16_workspace_bytes(*a), 'i8x3': lambda *a: lib.annlite_flat_search_i8_workspace_bytes(*a)}
    for name, code in _capi.FLAT_FILTER.items():
        for N, D, B, k in ((9000, 5, 130, 10), (1_000_000, 128, 1024, 64), (0, 33, 0, 1)):
            assert lib.annlite_flat_search_grouped_workspace_bytes(code, N, D, B, k, ctypes.byref(grouped)) == 0
            assert own[name](N, D, B, k, ctypes.byref(need)) == 0
            assert grouped.value == need.value > 0, (name, N, D, B, k)
    for bad in ((7, 100, 8, 4, 10), (-1, 100, 8, 4, 10), (0, 100, 8, 4, 65), (0, 100, 8, 4, 0), (0, 100, 0, 4, 10), (1, 100, 40000, 4, 10)):
        assert lib.annlite_flat_search_grouped_workspace_bytes(*bad, ctypes.byref(grouped)) != 0, bad
    assert lib.annlite_flat_search_grouped_workspace_bytes(0, 100, 8, 4, 10, None) != 0


def _search(lib, filter=0, metric=1, q=8, B=4, D=8, x=8, scale=1.0, norms=8, centre=None, N=100, valid=None, masks=8, ld=4, G=2, group=8, k=10,
            out_d=8, out_i=8, ws=8, ws_bytes=1 << 30):
    """``annlite_flat_search_topk_grouped`` with pointers that are never followed: every call here is refused by the checks"""
    return lib.annlite_flat_search_topk_grouped(filter, metric, q, B, D, x, scale, norms, centre, N, valid, masks, ld, G, group, k, 0, out_d, out_i,
                                                ws, ws_bytes, None)


def _stage(lib, filter=1, metric=1, q=8, B=4, D=8, x=8, scale=1.0, norms=8, centre=None, N=100, valid=None, masks=8, ld=4, G=2, group=8, stride=1,
           bounds=8, cand=8, count=8, scores=None, ws=8, ws_bytes=1 << 30):
    return lib.annlite_flat_filter_grouped(filter, metric, q, B, D, x, scale, norms, centre, N, valid, masks, ld, G, group, stride, bounds, cand,
                                           count, scores, ws, ws_bytes, None)


def test_the_entries_refuse_bad_arguments():
    _capi, lib = _lib()
    err = lambda: lib.annlite_hip_last_error().decode()
    for call in (_search, _stage):
        assert call(lib, G=0) != 0 and 'G' in err()
        assert call(lib, G=-3) != 0
        assert call(lib, ld=3) != 0 and 'mask_ld' in err()  # 96 bits for 100 rows
        assert call(lib, ld=-1) != 0
        assert call(lib, masks=None) != 0 and 'null' in err()
        assert call(lib, group=None) != 0 and 'null' in err()
        assert call(lib, filter=4) != 0 and 'filter' in err()
        assert call(lib, metric=0) != 0
        assert call(lib, D=0) != 0
        assert call(lib, filter=3, scale=3.0) != 0       # int8 rows: the scale is a power of two
        assert call(lib, filter=0, centre=8) != 0         # a centre is the split filter's
        assert call(lib, filter=1, metric=2, centre=8) != 0
        assert call(lib, ws_bytes=16) != 0 and 'workspace' in err()
        assert call(lib, B=0) == 0                        # nothing to do: nothing is read
    assert _search(lib, k=65) != 0 and _search(lib, k=0) != 0
    assert _stage(lib, stride=0) != 0
    assert _stage(lib, filter=0, scores=8) != 0 and 'scores' in err()  # (the f32 kernel has none)
    assert _stage(lib, N=0, ld=0) == 0
