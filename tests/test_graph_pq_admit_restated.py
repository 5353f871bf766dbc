"""The rule of the filtered PQ walk (annlite_graph_search_packed_admit), checked on its restatement without a GPU
(``_refs_pq_admit.walk_pq_admit_restated``; tests/test_graph_packed_admit.py pins the kernel to it), on a few hundred small random
graphs, for the one-at-a-time and the pair walk:

  * with every row admitted and ``ef = ef_route`` the result list R is the routing list C, and C is
    ``tests/test_graph_pair.py::walk_restated``'s list -- the filter adds a list, it does not change the walk;
  * under any filter the expansions, the rows evaluated and C itself are those of the walk without one;
  * R ends as the ``ef`` smallest (key, id) among the admitted rows ever offered, distinct and ascending, missing places at the tail;
  * a visited table that forgets changes nothing in R: a row offered again that is in R is dropped by the merge, one that is not lost
    against R's worst entry before, and that entry only falls.  With more seeds than C has places the argument is needed even when
    the table holds everything: a seed that missed C is not recorded as visited, may stand in R, and comes back as a neighbour.
"""
import numpy as np
import pytest

from _refs import key_to_bits, random_links
from _refs_pq_admit import pq_keys, walk_pq_admit_restated
from test_graph_pair import walk_restated as pair_walk_restated

N, M, KS = 400, 8, 256
# (L, ef_route, ef, seeds): every register count of both lists -- (1, 1), (2, 1), (2, 2), (3, 2), (3, 3) / (4, 2), (4, 4), (4, 1) --, a
# routing list of one place, more seeds than places
SHAPES = [(32, 64, 64, 40), (32, 128, 10, 100), (24, 128, 128, 100), (32, 160, 100, 100), (32, 192, 150, 150), (5, 256, 10, 30),
          (16, 256, 200, 70), (8, 1, 1, 3), (5, 10, 10, 150), (17, 33, 7, 65)]
GRAPHS_PER_SHAPE = 20


def _graph(shape, g):
    L, ef_route, ef, n_seeds = shape
    rs = np.random.RandomState(100003 * L + 1009 * ef_route + 31 * ef + g)
    links = random_links(rs, N, L).view(np.uint32)
    codes = rs.randint(0, KS, size=(N, M)).astype(np.uint8)
    codes[100:140] = codes[100]  # exact ties: the node id decides
    lut = rs.rand(M, KS).astype(np.float32)
    seeds = rs.choice(N, n_seeds, replace=False).astype(np.int32)
    admits = {'0.5': rs.rand(N) < 0.5, '0.1': rs.rand(N) < 0.1, 'one': np.arange(N) == int(seeds[0]), 'none': np.zeros(N, bool)}
    return links, codes, lut, seeds, admits


@pytest.mark.parametrize('shape', SHAPES)
def test_all_rows_admitted_and_ef_equal_to_ef_route_is_the_plain_walk(oracle, shape):
    L, ef_route, _, _ = shape
    for g in range(GRAPHS_PER_SHAPE):
        links, codes, lut, seeds, _ = _graph(shape, g)
        keys = pq_keys(oracle, lut, codes)
        for width in (1, 2):
            want_i, want_d = pair_walk_restated(oracle, links, seeds, codes, lut, ef_route, width)
            st = {}
            got_i, got_d = walk_pq_admit_restated(links, seeds, keys, ef_route, ef_route, np.ones(N, bool), width=width, stats=st)
            assert np.array_equal(got_i, want_i) and np.array_equal(got_d, want_d.view(np.uint32)), (g, width)
            assert np.array_equal(st['routing'][0], got_i) and np.array_equal(st['routing'][1], got_d), (g, width)  # R is C


@pytest.mark.parametrize('shape', SHAPES)
def test_result_list_is_the_best_admitted_rows_the_walk_evaluated(oracle, shape):
    L, ef_route, ef, _ = shape
    for g in range(GRAPHS_PER_SHAPE):
        links, codes, lut, seeds, admits = _graph(shape, g)
        keys = pq_keys(oracle, lut, codes)
        for width in (1, 2):
            plain = {}
            walk_pq_admit_restated(links, seeds, keys, ef_route, ef_route, np.ones(N, bool), width=width, stats=plain)
            for name, admit in admits.items():
                st = {}
                ids, dbits = walk_pq_admit_restated(links, seeds, keys, ef_route, ef, admit, width=width, stats=st)
                # the filter does not touch the routing
                assert (st['expansions'], st['evals']) == (plain['expansions'], plain['evals']), (g, width, name)
                assert st['route_worst_bits'] == plain['route_worst_bits'], (g, width, name)
                assert np.array_equal(st['routing'][0], plain['routing'][0]), (g, width, name)
                real = ids[ids >= 0]
                assert admit[real].all() and np.unique(real).size == real.size, (g, width, name)
                assert (ids[real.size:] == -1).all() and (dbits[real.size:] == 0x7f800000).all(), (g, width, name)  # missing: the tail
                pairs = [(int(keys[v]), int(v)) for v in real]
                assert pairs == sorted(pairs), (g, width, name)
                assert [key_to_bits(k) for k, _ in pairs] == [int(w) for w in dbits[:real.size]], (g, width, name)
                # the invariant
                best = sorted((int(keys[v]), v) for v in st['admitted_evaluated'])[:ef]
                assert pairs == best, (g, width, name)
                if name == 'none':
                    assert real.size == 0 and len(st['admitted_evaluated']) == 0
                if name == 'one':
                    assert real.size == 1 and real[0] == seeds[0]  # (a seed: the walk evaluates it)


@pytest.mark.parametrize('shape', SHAPES)
def test_a_forgetful_visited_table_returns_the_same_result_list(oracle, shape):
    L, ef_route, ef, _ = shape
    for g in range(0, GRAPHS_PER_SHAPE, 3):
        links, codes, lut, seeds, admits = _graph(shape, g)
        admits['all'] = np.ones(N, bool)
        keys = pq_keys(oracle, lut, codes)
        for width in (1, 2):
            for name, admit in admits.items():
                full = {}
                want_i, want_d = walk_pq_admit_restated(links, seeds, keys, ef_route, ef, admit, width=width, stats=full)
                for table in (0, 16, 64):
                    st = {}
                    got_i, got_d = walk_pq_admit_restated(links, seeds, keys, ef_route, ef, admit, width=width, table=table, stats=st)
                    assert np.array_equal(got_i, want_i) and np.array_equal(got_d, want_d), (g, width, name, table)
                    assert st['expansions'] == full['expansions'] and st['evals'] >= full['evals'], (g, width, name, table)
                    assert st['admitted_evaluated'] == full['admitted_evaluated'], (g, width, name, table)
                    assert st['route_worst_bits'] == full['route_worst_bits'], (g, width, name, table)


@pytest.mark.parametrize('width', [1, 2])
def test_the_result_list_needs_its_duplicate_check_even_with_a_table_that_holds_everything(oracle, width):
    """150 seeds, 10 places in C: admitted seeds that missed C stand in R and are met again as neighbours.  Without the merge's check
    R would list them twice -- shown here by counting how often an admitted row is offered."""
    shape = (5, 10, 10, 150)
    links, codes, lut, seeds, _ = _graph(shape, 0)
    keys = pq_keys(oracle, lut, codes)
    st = {}
    ids, _ = walk_pq_admit_restated(links, seeds, keys, 10, 10, np.ones(N, bool), width=width, stats=st)
    assert st['evals'] > len(st['admitted_evaluated'])  # some row was evaluated twice, with a table that holds everything
    real = ids[ids >= 0]
    assert real.size == 10 and np.unique(real).size == 10
