"""The argument the full-visited-table tests of tests/test_graph_f32_walk.py rest on, checked without a GPU: a walk whose visited
table forgets (Beam::visit once 16 buckets in a row are full: the node is reported as new every time) returns the list of the walk
whose table holds everything, PROVIDED the merge drops an offered (key, node) that is in the list already or came earlier in the
same offer -- and it does evaluate more rows, which is how the GPU test knows the path ran.  ``walk_forgetful`` is a second
restatement of the kernel's rule, written for the table that cannot record; ``walk_restated`` is the one the kernel is pinned to."""
import numpy as np
import pytest

from _refs import f32_key, random_links, walk_forgetful, walk_restated

N, N_SEEDS = 3000, 150
SHAPES = [(32, 64), (32, 128), (5, 10), (17, 33), (32, 200), (24, 256), (64, 100)]


def _key_vectors(rs):
    """Four queries' keys: three random ones, each with a run of 40 exact ties (the node id decides), and one all NaN."""
    d = rs.randn(4, N).astype(np.float32)
    d[1] = -np.abs(d[1])  # negative distances: the key, not the float's bits, orders them
    for b in range(3):
        d[b, 1000:1040] = np.sort(d[b])[5 + 10 * b]  # the ties stand near the front of the list: they are walked through
    d[3] = np.nan
    return f32_key(d)


@pytest.mark.parametrize('L,ef', SHAPES)
def test_a_forgetful_visited_table_returns_the_same_list(L, ef):
    rs = np.random.RandomState(1000 * L + ef)
    links = random_links(rs, N, L).view(np.uint32)
    seeds = rs.choice(N, N_SEEDS, replace=False).astype(np.int32)
    valid = rs.rand(N) < 0.9
    for b, keys in enumerate(_key_vectors(rs)):
        full = {}
        want_i, want_d = walk_restated(links, seeds, keys, ef, stats=full)
        masked_i, masked_d = walk_restated(links, seeds, keys, ef, valid)
        real = want_i[want_i >= 0]
        assert real.size == min(ef, 64 * (1 if ef <= 64 else 2 if ef <= 128 else 4)) and np.unique(real).size == real.size
        for table in (0, 16, 64, None):
            st = {}
            got_i, got_d = walk_forgetful(links, seeds, keys, ef, table, stats=st)
            assert np.array_equal(got_i, want_i) and np.array_equal(got_d, want_d), (b, table)
            assert st['expansions'] == full['expansions'], (b, table)
            if table is None:
                assert st['evals'] == full['evals'], b
            elif ef >= 64:
                assert st['evals'] > full['evals'], (b, table, st, full)  # (the nodes it forgot were evaluated again)
            else:
                assert st['evals'] >= full['evals'], (b, table)
        got_i, got_d = walk_forgetful(links, seeds, keys, ef, 16, valid)
        assert np.array_equal(got_i, masked_i) and np.array_equal(got_d, masked_d), b
