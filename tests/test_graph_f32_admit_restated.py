"""The rule of the filtered float walk (annlite_graph_f32_search_admit), checked on its restatement without a GPU
(``_refs_admit.walk_admit_restated``; tests/test_graph_f32_admit_walk.py pins the kernel to it):

  * the routing list C is ``_refs.walk_restated``'s at ``ef_route`` whatever the filter -- same expansions, same rows evaluated;
  * the result list R ends as the ``ef`` smallest (key, id) among the admitted rows the walk evaluated, distinct and ascending;
  * a visited table that forgets changes nothing in R -- the duplicate argument of tests/test_graph_f32_restated.py, for R: a row offered
    again that is in R is dropped by the merge, one that is not lost against R's worst entry before, and that entry only falls.  With
    150 seeds and fewer places in C the argument is needed even when the table holds everything: a seed that missed C is not recorded
    as visited, may stand in R, and comes back as somebody's neighbour.
"""
import numpy as np
import pytest

from _refs import f32_key, key_to_bits, random_links, walk_restated
from _refs_admit import walk_admit_restated

N, N_SEEDS = 3000, 150
SHAPES = [(32, 128, 64), (32, 64, 64), (5, 10, 10), (17, 33, 7), (32, 200, 129), (24, 256, 256), (64, 100, 1)]  # (L, ef_route, ef)
TIES = slice(1000, 1040)


def _key_vectors(rs):
    """Four queries' keys: three random ones, each with a run of 40 exact ties near the front of the list (the node id decides), one
    of them all negative, and one all NaN."""
    d = rs.randn(4, N).astype(np.float32)
    d[1] = -np.abs(d[1])
    for b in range(3):
        d[b, TIES] = np.sort(d[b])[5 + 10 * b]
    d[3] = np.nan
    return f32_key(d)


def _admits(rs):
    """density -> bool [N]: 0.5 and 0.05 at random (about half of the tie block admitted in each: every other row of it at 0.5, the
    first half at 0.05), exactly one row, none"""
    half = rs.rand(N) < 0.5
    half[TIES] = np.arange(40) % 2 == 0
    sparse = rs.rand(N) < 0.05
    sparse[TIES] = np.arange(40) < 20
    one = np.zeros(N, bool)
    one[1010] = True  # (inside the tie block: the walk reaches it)
    return {'0.5': half, '0.05': sparse, 'one': one, 'none': np.zeros(N, bool)}


def _graph(L, ef_route, ef):
    rs = np.random.RandomState(1000 * L + ef_route + 7 * ef)
    links = random_links(rs, N, L).view(np.uint32)
    seeds = rs.choice(N, N_SEEDS, replace=False).astype(np.int32)
    return rs, links, seeds


@pytest.mark.parametrize('L,ef', [(L, er) for L, er, _ in SHAPES])
def test_all_rows_admitted_and_ef_equal_to_ef_route_is_the_plain_walk(L, ef):
    rs, links, seeds = _graph(L, ef, ef)
    for keys in _key_vectors(rs):
        want_i, want_d = walk_restated(links, seeds, keys, ef)
        got_i, got_d = walk_admit_restated(links, seeds, keys, ef, ef, np.ones(N, bool))
        assert np.array_equal(got_i, want_i) and np.array_equal(got_d, want_d)


@pytest.mark.parametrize('L,ef_route,ef', SHAPES)
def test_result_list_is_the_best_admitted_rows_the_walk_evaluated(L, ef_route, ef):
    rs, links, seeds = _graph(L, ef_route, ef)
    admits = _admits(rs)
    for b, keys in enumerate(_key_vectors(rs)):
        plain = {}
        walk_restated(links, seeds, keys, ef_route, stats=plain)
        for name, admit in admits.items():
            st = {}
            ids, dbits = walk_admit_restated(links, seeds, keys, ef_route, ef, admit, stats=st)
            # the filter does not touch the routing
            assert (st['expansions'], st['evals']) == (plain['expansions'], plain['evals']), (b, name)
            real = ids[ids >= 0]
            assert admit[real].all() and np.unique(real).size == real.size, (b, name)
            assert (ids[real.size:] == -1).all() and (dbits[real.size:] == 0x7f800000).all(), (b, name)  # missing places: at the tail
            pairs = [(int(keys[v]), int(v)) for v in real]
            assert pairs == sorted(pairs), (b, name)
            assert [key_to_bits(k) for k, _ in pairs] == [int(w) for w in dbits[:real.size]], (b, name)
            # the invariant
            best = sorted((int(keys[v]), v) for v in st['admitted_evaluated'])[:ef]
            assert pairs == best, (b, name)
            if name == 'none':
                assert real.size == 0
            if name == 'one':
                assert real.size <= 1
        assert len(st['admitted_evaluated']) == 0  # ('none' ran last)


@pytest.mark.parametrize('L,ef_route,ef', SHAPES)
def test_a_forgetful_visited_table_returns_the_same_result_list(L, ef_route, ef):
    rs, links, seeds = _graph(L, ef_route, ef)
    admits = _admits(rs)
    admits['all'] = np.ones(N, bool)
    for b, keys in enumerate(_key_vectors(rs)):
        for name, admit in admits.items():
            full = {}
            want_i, want_d = walk_admit_restated(links, seeds, keys, ef_route, ef, admit, stats=full)
            for table in (0, 16, 64):
                st = {}
                got_i, got_d = walk_admit_restated(links, seeds, keys, ef_route, ef, admit, table=table, stats=st)
                assert np.array_equal(got_i, want_i) and np.array_equal(got_d, want_d), (b, name, table)
                assert st['expansions'] == full['expansions'] and st['evals'] >= full['evals'], (b, name, table)
                assert st['admitted_evaluated'] == full['admitted_evaluated'], (b, name, table)


def test_the_result_list_needs_its_duplicate_check_even_with_a_table_that_holds_everything():
    """150 seeds, 10 places in C: admitted seeds that missed C stand in R and are met again as neighbours.  Without the merge's check
    R would list them twice -- shown here by counting how often an admitted row is offered."""
    L, ef_route, ef = 5, 10, 10
    rs, links, seeds = _graph(L, ef_route, ef)
    keys = _key_vectors(rs)[0]
    admit = np.ones(N, bool)
    st = {}
    ids, _ = walk_admit_restated(links, seeds, keys, ef_route, ef, admit, stats=st)
    plain = {}
    walk_restated(links, seeds, keys, ef_route, stats=plain)
    assert plain['evals'] > len(st['admitted_evaluated'])  # some row was evaluated twice, with a full table
    real = ids[ids >= 0]
    assert real.size == ef and np.unique(real).size == ef
