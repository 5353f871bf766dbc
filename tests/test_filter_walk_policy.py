"""The filter policy of the two HNSW indexes (annlite_amd/core/index/filter_walk.py) on CPU tensors, without a GPU: the two pure
functions -- places of the routing list, queries to answer again -- and the skeleton of ``_search_filtered_on_graph`` over a stub
parent and stub hooks."""
import numpy as np
import pytest
import torch

from annlite_amd.core.index.filter_walk import FilterWalkMixin, queries_to_reanswer, routing_places

INF = float('inf')


@pytest.mark.parametrize('ef, n_adm, places', [(50, 1000, 50), (50, 500, 100), (50, 300, 167), (50, 1, 256), (200, 999, 201)])
def test_routing_places(ef, n_adm, places):
    assert routing_places(ef, 1000, n_adm, 256) == places


def test_queries_to_reanswer():
    cand = torch.tensor([[3, 5, 7, 9],      # a full list within reach
                         [3, -1, -1, -1],   # -1 at depth - 1 (depth 2 and depth 4)
                         [3, 5, 7, 9],      # its entries at depth - 1 lie beyond reach
                         [3, 5, 7, 9]])     # reach = +inf: the routing list never filled
    cand_d = torch.tensor([[.1, .2, .3, .4], [.1, INF, INF, INF], [.1, .6, .7, .8], [.1, .2, .3, .4]])
    reach = torch.tensor([.4, .9, .5, INF])
    for depth in (2, 4):
        assert queries_to_reanswer(cand, cand_d, reach, depth).tolist() == [1, 2]


class _Parent:
    """What the mixin asks of the index below it, on the host."""
    MAX_EF = 256
    FILTER_WALK_MIN_FRACTION = 0.1

    def __init__(self, n_rows):
        self._n_rows = n_rows
        self.exact_calls = []

    def _filter_bits(self, indices):
        sel = torch.zeros(self._n_rows, dtype=torch.bool)
        sel[torch.as_tensor(list(indices), dtype=torch.int64)] = True
        return sel

    @staticmethod
    def _unpack_bits(bits, n):
        return bits[:n]

    def _pre(self, x):
        return torch.as_tensor(x, dtype=torch.float32).reshape(-1, 2)

    def _to_dev(self, a):
        return torch.as_tensor(a)

    def search_batch(self, x, limit=10, indices=None):
        self.exact_calls.append(np.asarray(x).copy())
        B = len(x)
        return np.full((B, limit), 9.0, np.float32), np.full((B, limit), 99, np.int64)


class _Index(FilterWalkMixin, _Parent):
    def __init__(self, n_rows, filter_search='graph'):
        _Parent.__init__(self, n_rows)
        self._init_filter_search(filter_search)
        self.walks = []

    def _filter_walk(self, q, ef_route, ef, admit, reach):
        self.walks.append((ef_route, ef))
        B = q.shape[0]
        reach[:] = 1.0
        cand = torch.arange(ef, dtype=torch.int64)[None, :].repeat(B, 1)
        cand_d = torch.linspace(0.0, 0.5, ef)[None, :].repeat(B, 1)
        cand[B - 1, 1:], cand_d[B - 1, 1:] = -1, INF  # the last query's list holds one row
        return cand, cand_d

    def _filter_rank(self, x, q, cand, cand_d, k, ef, admit):
        return cand_d[:, :k].clone(), cand[:, :k].clone(), k


def test_skeleton_floor_order_and_reanswer():
    ix = _Index(1000)
    x = np.arange(6, dtype=np.float32).reshape(3, 2)
    assert ix._filtered_answer(x, 2, 4, [], None, True) is None  # no admitted row
    assert ix._filtered_answer(x, 2, 4, range(50), None, True) is None  # below the floor, the constructor's rule
    assert ix.last_filter_path == 'exact' and not ix.walks
    assert ix._filtered_answer(x, 2, 4, range(500), 'graph', False) is None  # the index's own test says no walk
    d, i = ix._filtered_answer(x, 2, 4, range(50), 'graph', True)  # below the floor, ordered: it walks
    assert ix.walks == [(80, 4)] and ix.last_filter_path == 'graph'
    assert isinstance(d, np.ndarray) and i[:2].tolist() == [[0, 1], [0, 1]]
    # the short query was answered again by the parent, from the caller's own row
    assert ix.last_filter_reanswered == 1 and i[2].tolist() == [99, 99] and d[2].tolist() == [9.0, 9.0]
    assert len(ix.exact_calls) == 1 and np.array_equal(ix.exact_calls[0], x[2:3])
    assert _Index(1000, 'exact')._filtered_answer(x, 2, 4, range(500), None, True) is None


def test_filter_search_values_are_checked():
    ix = _Index(10)
    ix._check_filter_search(None)
    ix._check_filter_search('graph')
    with pytest.raises(ValueError, match='filter_search'):
        ix._check_filter_search('walk')
    with pytest.raises(ValueError, match='the filtered walk'):
        ix._check_filter_search(None, 'the exact search')  # (the constructor's value has to be one of the two)
