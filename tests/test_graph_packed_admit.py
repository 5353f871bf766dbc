"""The filtered PQ walk (annlite_graph_search_packed_admit, graph_admit.hip) pinned BIT FOR BIT -- ids, distance bits and the routing
list's last sum -- against its restatement (``_refs_pq_admit``, itself checked without a GPU in tests/test_graph_pq_admit_restated.py):
a routing list that is the packed walk's at ``ef_route`` whatever the filter, one node or two per step, and a result list that keeps the
``ef`` best admitted rows among everything the walk evaluates.  Sums are hnswlib::PQLookup through the oracle's ``adc_gather_c``.

tests/test_graph_pair.py's construction: 6000 rows, 10 queries, Ks = 256, 150 seeds, its random link lists (ids beyond the table, a
neighbour listed twice), a block of 40 identical code rows for exact ties.  Every case runs five filters -- every row, half, a tenth,
a hundredth, none -- and both widths.  Beyond that: 1, 65 and 300 seeds against 64 routing places (a seed that missed the routing list
stands in the result list and comes back as a neighbour), seeds beyond the table, one query, a table of one row, no query, visited
tables of 16 and 64 entries, the walk's counters against the plain packed walk's, and what the library refuses."""
import numpy as np
import pytest

from _refs import bitmap
from _refs_pq_admit import INF_BITS, ResultList, pq_keys, walk_pq_restated
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

N, B, KS, N_SEEDS = 6000, 10, 256, 150
DENSITIES = ('1.0', '0.5', '0.1', '0.01', 'none')
TIES = slice(1000, 1040)


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _random_graph(rs, N, L, full_frac=0.6):
    """tests/test_graph_pair.py's link lists"""
    links = np.zeros((N, L + 1), np.uint32)
    cnt = np.where(rs.rand(N) < full_frac, L, rs.randint(0, L + 1, N)).astype(np.uint32)
    links[:, 0] = cnt
    nb = rs.randint(0, N, size=(N, L)).astype(np.uint32)
    near = (np.arange(N)[:, None] + rs.randint(1, 50, size=(N, L))) % N
    nb = np.where(rs.rand(N, L) < 0.7, near, nb).astype(np.uint32)
    nb[rs.rand(N, L) < 0.002] = N + 5  # beyond the table: never followed
    nb[:, 1] = np.where(rs.rand(N) < 0.05, nb[:, 0], nb[:, 1])  # a neighbour listed twice
    links[:, 1:] = nb
    return links.view(np.int32)


class _Case:
    pass


_cases = {}


def _case(ops, oracle, M, L, b=B, seeds='150'):
    """Made once per shape and left unchanged: table, tables of the queries, link lists, seeds ('150' distinct ids, '1' / '65' / '300'
    of them, or 'beyond': every fifth id >= N), the five filters (the tie block partly admitted), the packed records, and per query
    the key of its sum to every row."""
    key = (M, L, b, seeds)
    if key in _cases:
        return _cases[key]
    rs = np.random.RandomState(M * 1000 + L * 7 + 31 * b + len(seeds) + 5)
    c = _Case()
    c.M, c.L, c.b = M, L, b
    c.links = _random_graph(rs, N, L)
    c.codes = rs.randint(0, KS, size=(N, M)).astype(np.uint8)
    c.codes[TIES] = c.codes[TIES.start]  # exact ties inside the walk: the key's low word (the node id) decides
    c.lut = rs.rand(b, M, KS).astype(np.float32)
    n_seeds = N_SEEDS if seeds in ('150', 'beyond') else int(seeds)
    c.seeds = rs.choice(N, n_seeds, replace=False).astype(np.int64)
    if seeds == 'beyond':
        c.seeds[::5] = N + np.arange(c.seeds[::5].size) * 7
        c.seeds[5] = 0xfffffffe
    c.seeds = c.seeds.astype(np.uint32)
    half = rs.rand(N) < 0.5
    half[TIES] = np.arange(40) % 2 == 0
    tenth = rs.rand(N) < 0.1
    tenth[TIES] = np.arange(40) < 20
    c.admit = {'1.0': np.ones(N, bool), '0.5': half, '0.1': tenth, '0.01': rs.rand(N) < 0.01, 'none': np.zeros(N, bool)}
    c.admit_d = {name: ops.to_dev(bitmap(a)) for name, a in c.admit.items()}
    c.links_d, c.codes_d, c.lut_d = ops.to_dev(c.links), ops.to_dev(c.codes), ops.to_dev(c.lut)
    c.seeds_d = ops.to_dev(c.seeds.view(np.int32))
    c.packed = ops.graph_pack(c.links_d, c.codes_d)
    c.keys = [pq_keys(oracle, c.lut[q], c.codes) for q in range(b)]
    c.restated = {}
    _cases[key] = c
    return c


def _restated(c, ef_route, ef, width):
    """density -> (ids [b, ef], bits [b, ef]) and the walk's totals, once per (case, list sizes, width): the five filters ride one walk"""
    k = (ef_route, ef, width)
    if k not in c.restated:
        lk = c.links.view(np.uint32)
        tot = dict(expansions=0, evals=0, route_worst_bits=[])
        out = {name: ([], []) for name in DENSITIES}
        for q in range(c.b):
            lists = {name: ResultList(ef, c.admit[name], width) for name in DENSITIES}
            st = {}
            walk_pq_restated(lk, c.seeds, c.keys[q], ef_route, list(lists.values()), width=width, stats=st)
            tot['expansions'] += st['expansions']
            tot['evals'] += st['evals']
            tot['route_worst_bits'].append(st['route_worst_bits'])
            for name, r in lists.items():
                i, d = r.output()
                out[name][0].append(i)
                out[name][1].append(d)
        tot['route_worst_bits'] = np.array(tot['route_worst_bits'], np.uint32)
        c.restated[k] = ({name: (np.stack(v[0]), np.stack(v[1])) for name, v in out.items()}, tot)
    return c.restated[k]


def _run(ops, c, ef_route, ef, density, width, reach=None):
    """``reach``: a list that receives the routing list's last sum per query (bits)"""
    import torch

    rw = None if reach is None else torch.full((c.b,), -1.0, dtype=torch.float32, device='cuda')
    gi, gd = ops.graph_search_packed_admit(c.packed, c.L, c.seeds_d, c.codes_d, c.lut_d, ef_route, ef, c.admit_d[density],
                                           expand_width=width, route_worst=rw)
    torch.cuda.synchronize()
    if reach is not None:
        reach.append(rw.cpu().numpy().view(np.uint32))
    return gi.cpu().numpy(), gd.cpu().numpy().view(np.uint32)


def _assert_equals_restated(ops, c, ef_route, ef, widths=(1, 2), densities=DENSITIES):
    for width in widths:
        want, tot = _restated(c, ef_route, ef, width)
        for density in densities:
            wi, wbits = want[density]
            reach = []
            gi, gbits = _run(ops, c, ef_route, ef, density, width, reach)
            assert gi.shape == (c.b, ef) and gbits.shape == (c.b, ef)
            assert np.array_equal(reach[0], tot['route_worst_bits']), (width, density)  # how far the walk reached: the filter does not move it
            for q in range(c.b):
                assert np.array_equal(gi[q], wi[q]), (width, density, q)
                assert np.array_equal(gbits[q], wbits[q]), (width, density, q)
            real = gi >= 0
            assert c.admit[density][gi[real]].all(), (width, density)  # admitted rows only
            if density == 'none':
                assert (gi == -1).all() and (gbits == INF_BITS).all()


# every M; L = 32, 24, 5 under both widths, L = 40 (records of more than a half wave) one node at a time; every pair of list sizes:
# registers per lane (E, ER) = (1, 1), (2, 1), (2, 2), (3, 1) / (4, 1), (3, 2) / (4, 2), (4, 1), (4, 3) / (4, 4), and one place each
SHAPES = [(16, 32, 64, 64, (1, 2)), (16, 32, 128, 10, (1, 2)), (8, 32, 128, 128, (1, 2)), (32, 24, 160, 64, (1, 2)),
          (16, 24, 192, 100, (1, 2)), (64, 32, 256, 10, (1, 2)), (8, 5, 256, 200, (1, 2)), (16, 5, 1, 1, (1, 2)),
          (32, 32, 128, 128, (1, 2)), (64, 24, 64, 64, (1, 2)), (64, 5, 192, 100, (1, 2)), (32, 5, 256, 200, (1, 2)),
          (16, 40, 128, 10, (1,)), (8, 40, 256, 200, (1,))]


@pytest.mark.parametrize('M,L,ef_route,ef,widths', SHAPES)
def test_filtered_walk_equals_its_restatement(ops, oracle, M, L, ef_route, ef, widths):
    _assert_equals_restated(ops, _case(ops, oracle, M, L), ef_route, ef, widths)


@pytest.mark.parametrize('M,L,ef_route', [(16, 32, 128), (8, 5, 64), (32, 24, 160), (64, 32, 256)])
def test_all_rows_admitted_at_ef_route_is_the_plain_packed_walk(ops, oracle, M, L, ef_route):
    """ef = ef_route, every row admitted: the result list is annlite_graph_search_packed_ex's list."""
    import torch

    c = _case(ops, oracle, M, L)
    for width in (1, 2):
        gi, gbits = _run(ops, c, ef_route, ef_route, '1.0', width)
        pi, pd = ops.graph_search_packed(c.packed, L, c.seeds_d, c.codes_d, c.lut_d, ef_route, expand_width=width)
        torch.cuda.synchronize()
        assert np.array_equal(gi, pi.cpu().numpy()) and np.array_equal(gbits, pd.cpu().numpy().view(np.uint32)), width


@pytest.mark.parametrize('seeds', ['1', '65', '300', 'beyond'])
def test_filtered_walk_seed_sets(ops, oracle, seeds):
    """64 routing places: 65 and 300 seeds are more than the routing list holds (the result list checks for copies from the start)."""
    c = _case(ops, oracle, 16, 32, seeds=seeds)
    if seeds == 'beyond':
        assert (c.seeds.astype(np.int64) >= N).sum() == N_SEEDS // 5
    _assert_equals_restated(ops, c, 64, 64)
    _assert_equals_restated(ops, c, 64, 10)
    gi, _ = _run(ops, c, 64, 64, '0.5', 2)
    assert (gi >= 0).sum(1).min() == 64  # (the walk went somewhere: a full list of admitted rows)


@pytest.mark.parametrize('width', [1, 2])
def test_a_seed_that_missed_the_routing_list_stands_in_the_result_list_and_comes_back(ops, oracle, width):
    """300 seeds, 64 routing places.  Query 0's WORST seed misses the routing list -- it is not recorded as visited -- but it is the only
    admitted row beside a handful, so it stands in the result list; the query's BEST seed, expanded first, lists it as a neighbour.  The
    walk evaluates it again and offers it again: the result list holds it once."""
    import torch

    base = _case(ops, oracle, 16, 32, seeds='300')
    order = np.argsort(base.keys[0][base.seeds.astype(np.int64)], kind='stable')
    best, worst = int(base.seeds[order[0]]), int(base.seeds[order[-1]])
    links = base.links.copy().view(np.uint32)
    links[best, 0] = max(int(links[best, 0]), 2)
    links[best, 2] = worst
    admit = np.zeros(N, bool)
    admit[[worst, 7, 2000, 4500]] = True
    r = ResultList(10, admit, width)
    st = {}
    walk_pq_restated(links, base.seeds, base.keys[0], 64, [r], width=width, stats=st)
    assert worst not in st['routing'][0] and r.offered[worst] >= 2  # missed C, offered as a seed and again as a neighbour
    wi, wbits = r.output()
    assert (wi == worst).sum() == 1
    links_d = ops.to_dev(links.view(np.int32))
    packed = ops.graph_pack(links_d, base.codes_d)
    gi, gd = ops.graph_search_packed_admit(packed, 32, base.seeds_d, base.codes_d, base.lut_d[:1].contiguous(), 64, 10,
                                           ops.to_dev(bitmap(admit)), expand_width=width)
    torch.cuda.synchronize()
    assert np.array_equal(gi.cpu().numpy()[0], wi) and np.array_equal(gd.cpu().numpy().view(np.uint32)[0], wbits)


def test_filtered_walk_with_one_query(ops, oracle):
    _assert_equals_restated(ops, _case(ops, oracle, 16, 32, b=1), 128, 64)


@pytest.mark.parametrize('admitted', [True, False])
def test_filtered_walk_over_one_row(ops, oracle, admitted):
    import torch

    M = 8
    codes = np.arange(M, dtype=np.uint8)[None, :]
    lut = np.random.RandomState(3).rand(2, M, KS).astype(np.float32)
    links = np.zeros((1, 9), np.int32)
    seeds = np.zeros(1, np.int32)
    admit = np.array([admitted])
    links_d, codes_d = ops.to_dev(links), ops.to_dev(codes)
    packed = ops.graph_pack(links_d, codes_d)
    for width in (1, 2):
        gi, gd = ops.graph_search_packed_admit(packed, 8, ops.to_dev(seeds), codes_d, ops.to_dev(lut), 10, 4, ops.to_dev(bitmap(admit)),
                                               expand_width=width)
        torch.cuda.synchronize()
        gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
        for q in range(2):
            r = ResultList(4, admit, width)
            walk_pq_restated(links.view(np.uint32), seeds, pq_keys(oracle, lut[q], codes), 10, [r], width=width)
            ri, rbits = r.output()
            assert np.array_equal(gi[q], ri) and np.array_equal(gd[q].view(np.uint32), rbits)
            assert list(gi[q]) == [0 if admitted else -1, -1, -1, -1]


def test_filtered_walk_with_no_query(ops, oracle):
    import torch

    c = _case(ops, oracle, 16, 32)
    gi, gd = ops.graph_search_packed_admit(c.packed, 32, c.seeds_d, c.codes_d, c.lut_d[:0].contiguous(), 64, 10, c.admit_d['0.5'])
    torch.cuda.synchronize()
    assert gi.shape == (0, 10) and gd.shape == (0, 10)


# (registers per lane of the routing and of the result list: (1, 1), (2, 1), (2, 2), (4, 4) / (3, 3), (4, 2), (4, 1))
SMALL_TABLE = [(16, 32, 64, 64), (16, 32, 128, 10), (8, 32, 128, 128), (16, 24, 192, 150), (32, 24, 256, 100), (64, 32, 256, 10)]


@pytest.mark.parametrize('hash_bits', [4, 6])
@pytest.mark.parametrize('M,L,ef_route,ef', SMALL_TABLE)
def test_a_full_visited_table_changes_nothing_in_the_result_list(ops, oracle, monkeypatch, M, L, ef_route, ef, hash_bits):
    """ANNLITE_GRAPH_HASH_BITS = 4 / 6 (16 / 64 visited entries): every neighbour is reported as new, evaluated again and offered to
    both lists again.  The result list is the default table's and the restatement's, no id twice; the counters show that the path ran:
    the expansions of the default table, more rows evaluated."""
    from annlite_amd import _capi

    c = _case(ops, oracle, M, L)
    for width in (1, 2):
        default = {density: _run(ops, c, ef_route, ef, density, width) for density in ('0.5', '1.0')}
        monkeypatch.setenv('ANNLITE_DEBUG_COUNTERS', '1')
        _run(ops, c, ef_route, ef, '0.5', width)
        large = _capi.graph_search_stats_ex()
        monkeypatch.delenv('ANNLITE_DEBUG_COUNTERS')
        monkeypatch.setenv('ANNLITE_GRAPH_HASH_BITS', str(hash_bits))
        want, tot = _restated(c, ef_route, ef, width)
        for density in ('0.5', '1.0'):
            wi, wbits = want[density]
            gi, gbits = _run(ops, c, ef_route, ef, density, width)
            for q in range(c.b):
                assert np.array_equal(gi[q], wi[q]) and np.array_equal(gbits[q], wbits[q]), (width, density, q)
                real = gi[q][gi[q] >= 0]
                assert np.unique(real).size == real.size
            assert np.array_equal(gi, default[density][0]) and np.array_equal(gbits, default[density][1]), (width, density)
        monkeypatch.setenv('ANNLITE_DEBUG_COUNTERS', '1')
        _run(ops, c, ef_route, ef, '0.5', width)
        small = _capi.graph_search_stats_ex()
        monkeypatch.delenv('ANNLITE_DEBUG_COUNTERS')
        monkeypatch.delenv('ANNLITE_GRAPH_HASH_BITS')
        print(f'width={width} hash_bits={hash_bits} (expansions, rows, prefetch hits): small table {small}, default table {large}, '
              f"restated ({tot['expansions']}, {tot['evals']})")
        assert small[0] == large[0] == tot['expansions']
        assert large[1] == tot['evals']
        assert small[1] > large[1]


@pytest.mark.parametrize('M,L,ef_route,ef', [(16, 32, 128, 64), (8, 24, 192, 10), (64, 5, 256, 200)])
def test_the_filter_does_not_route(ops, oracle, monkeypatch, M, L, ef_route, ef):
    """Expansions, rows evaluated and prefetched records used are the plain packed walk's at ``ef_route`` under every filter, for both
    widths."""
    import torch
    from annlite_amd import _capi

    c = _case(ops, oracle, M, L)
    monkeypatch.setenv('ANNLITE_DEBUG_COUNTERS', '1')
    for width in (1, 2):
        ops.graph_search_packed(c.packed, L, c.seeds_d, c.codes_d, c.lut_d, ef_route, expand_width=width)
        torch.cuda.synchronize()
        plain = _capi.graph_search_stats_ex()
        tot = _restated(c, ef_route, ef, width)[1]
        assert plain[:2] == (tot['expansions'], tot['evals']), width
        for density in DENSITIES:
            _run(ops, c, ef_route, ef, density, width)
            assert _capi.graph_search_stats_ex() == plain, (width, density)


def test_filtered_walk_refuses_what_it_cannot_hold(ops):
    """ef > ef_route, ef_route beyond 256, a missing bitmap and the pair walk over records of more than 32 neighbours are refused by the
    library's parameter checks: nothing is launched."""
    import torch

    rs = np.random.RandomState(1)
    n, M = 500, 16
    codes = ops.to_dev(rs.randint(0, KS, size=(n, M)).astype(np.uint8))
    lut = ops.to_dev(rs.rand(2, M, KS).astype(np.float32))
    seeds = ops.to_dev(np.arange(10, dtype=np.int32))
    admit = ops.to_dev(bitmap(np.ones(n, bool)))
    packed = {L: ops.graph_pack(ops.to_dev(_random_graph(rs, n, L)), codes) for L in (8, 40)}
    with pytest.raises(Exception, match='ef_route'):
        ops.graph_search_packed_admit(packed[8], 8, seeds, codes, lut, 16, 17, admit)
    with pytest.raises(Exception, match='ef_route'):
        ops.graph_search_packed_admit(packed[8], 8, seeds, codes, lut, 257, 16, admit)
    with pytest.raises(Exception, match='admit_bits'):
        ops.graph_search_packed_admit(packed[8], 8, seeds, codes, lut, 16, 16, None)
    with pytest.raises(Exception, match='width'):
        ops.graph_search_packed_admit(packed[40], 40, seeds, codes, lut, 32, 16, admit, expand_width=2)
    with pytest.raises(Exception, match='width'):
        ops.graph_search_packed_admit(packed[8], 8, seeds, codes, lut, 32, 16, admit, expand_width=3)
    gi, _ = ops.graph_search_packed_admit(packed[40], 40, seeds, codes, lut, 32, 16, admit, expand_width=1)
    torch.cuda.synchronize()
    assert (gi.cpu().numpy() >= 0).all()
