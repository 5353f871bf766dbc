"""The filtered float walk (annlite_graph_f32_search_admit, graph_f32.hip) pinned BIT FOR BIT against its restatement
(``_refs_admit.walk_admit_restated``, itself checked without a GPU in tests/test_graph_f32_admit_restated.py): a routing list that is
the plain walk's at ``ef_route`` whatever the filter, and a result list that keeps the ``ef`` best admitted rows among everything the
walk evaluates.  As in tests/test_graph_f32_walk.py the oracle distances are ``ops.exact_gather_dist``'s over all rows and the lists
are ordered by (``f32_key(distance)``, node id).

Every case runs five filters: half of the rows, one in twenty, all, none (every output (-1, +inf)) and exactly one row; the block of 40
exact ties is admitted in part.  Beyond the comfortable shapes: visited tables of 16 and 64 entries at one, two and four registers per
lane (rows are evaluated and offered to the result list again and again: its merge has to drop them), 150 seeds against a routing
list of 10 or 33 places (a seed that missed the routing list stands in the result list and comes back as a neighbour), D = 1 and
D = 2048, B = 1, one seed, 65 seeds, seeds beyond the table, tables of no row and of one row."""
import numpy as np
import pytest

from _refs import bitmap, f32_key, random_links, walk_restated
from _refs_admit import walk_admit_restated
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

EUCLIDEAN, INNER_PRODUCT, COSINE = 1, 2, 3
N, B, N_SEEDS = 3000, 10, 150
DENSITIES = ('0.5', '0.05', 'all', 'none', 'one')


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


class _Case:
    pass


_cases = {}


def _case(ops, metric, D, L, n=N, b=B, seeds='150'):
    """A table of ``n`` rows with a block of 40 exact ties, ``b`` queries -- a stored row as its own query, a NaN and an inf query
    where the batch has them --, random link lists (a neighbour listed twice, ids beyond the table), the seeds ('150' distinct ids,
    '1' / '65' of them, or 'beyond': every fifth id >= n), the five filters, and the distance matrix of ``exact_gather_dist`` with its
    keys.  Made once per shape and left unchanged."""
    import torch

    key = (metric, D, L, n, b, seeds)
    if key in _cases:
        return _cases[key]
    rs = np.random.RandomState(metric * 100003 + D * 1000 + L * 7 + n + 31 * b + 5)
    c = _Case()
    c.metric, c.D, c.L, c.n, c.b = metric, D, L, n, b
    c.links = random_links(rs, n, L)
    c.x = rs.randn(n, D).astype(np.float32)
    t0 = n // 3
    c.x[t0:t0 + 40] = c.x[t0]
    c.q = rs.randn(b, D).astype(np.float32)
    c.self_q, c.self_row = min(2, b - 1), 77
    c.q[c.self_q] = c.x[c.self_row]
    if metric == COSINE:
        c.x /= np.linalg.norm(c.x, axis=1, keepdims=True)
        c.q /= np.linalg.norm(c.q, axis=1, keepdims=True)
    if b > 7:
        c.q[4, D // 2] = np.nan
        c.q[7, 0] = np.inf
    full = np.nonzero(c.links.view(np.uint32)[:, 0] == L)[0]
    n_seeds = N_SEEDS if seeds in ('150', 'beyond') else int(seeds)
    c.seeds = rs.choice(full, n_seeds, replace=False).astype(np.int64)
    if seeds == 'beyond':
        c.seeds[::5] = n + np.arange(c.seeds[::5].size) * 7
        c.seeds[5] = 0xfffffffe
    if n_seeds >= 64 and c.self_row not in c.seeds:
        c.seeds[1] = c.self_row  # (random links, not a proximity graph: the row that is its own query is a seed)
    c.seeds = c.seeds.astype(np.uint32)
    c.one_row = c.self_row if n_seeds >= 64 else int(c.seeds[0])
    half = rs.rand(n) < 0.5
    half[t0:t0 + 40] = np.arange(40) % 2 == 0   # the tie block partly admitted
    sparse = rs.rand(n) < 0.05
    sparse[t0:t0 + 40] = np.arange(40) < 20
    one = np.zeros(n, bool)
    one[c.one_row] = True                       # (a seed: the walk evaluates it)
    c.admit = {'0.5': half, '0.05': sparse, 'all': np.ones(n, bool), 'none': np.zeros(n, bool), 'one': one}
    c.admit_d = {name: ops.to_dev(bitmap(a)) for name, a in c.admit.items()}
    c.x_d, c.q_d, c.links_d, c.seeds_d = ops.to_dev(c.x), ops.to_dev(c.q), ops.to_dev(c.links), ops.to_dev(c.seeds)
    all_rows = torch.arange(n, device='cuda', dtype=torch.int64)[None, :].expand(b, n).contiguous()
    c.dist = ops.exact_gather_dist(metric, c.q_d, c.x_d, all_rows).cpu().numpy()
    if b > 7:
        assert np.isnan(c.dist[4]).all() and not np.isfinite(c.dist[7]).any()
    c.keys = f32_key(c.dist)
    c.restated = {}
    _cases[key] = c
    return c


def _restated(c, ef_route, ef, density):
    """([ids per query], [bits per query]) of the restatement and its counters summed over the batch, once per (case, list sizes, filter)"""
    k = (ef_route, ef, density)
    if k not in c.restated:
        lk = c.links.view(np.uint32)
        tot = dict(expansions=0, evals=0)
        rows, reach = [], []
        for b in range(c.b):
            st = {}
            rows.append(walk_admit_restated(lk, c.seeds, c.keys[b], ef_route, ef, c.admit[density], stats=st))
            tot = {name: tot[name] + st[name] for name in tot}
            reach.append(st['route_worst_bits'])
        tot['route_worst_bits'] = np.array(reach, np.uint32)
        c.restated[k] = (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), tot)
    return c.restated[k]


def _run(ops, c, ef_route, ef, density, reach=None):
    """``reach``: a list that receives the routing list's last distance per query (bits)"""
    import torch

    rw = None if reach is None else torch.full((c.b,), -1.0, dtype=torch.float32, device='cuda')
    gi, gd = ops.graph_f32_search_admit(c.metric, c.q_d, c.x_d, c.links_d, c.seeds_d, ef_route, ef, c.admit_d[density], route_worst=rw)
    torch.cuda.synchronize()
    if reach is not None:
        reach.append(rw.cpu().numpy().view(np.uint32))
    return gi.cpu().numpy(), gd.cpu().numpy().view(np.uint32)


def _assert_equals_restated(ops, c, ef_route, ef, densities=DENSITIES):
    for density in densities:
        wi, wbits, tot = _restated(c, ef_route, ef, density)
        reach = []
        gi, gbits = _run(ops, c, ef_route, ef, density, reach)
        assert gi.shape == (c.b, ef) and gbits.shape == (c.b, ef)
        assert np.array_equal(reach[0], tot['route_worst_bits']), density  # how far the walk reached: the filter does not move it
        for b in range(c.b):
            assert np.array_equal(gi[b], wi[b]), (density, b)
            assert np.array_equal(gbits[b], wbits[b]), (density, b)
        real = gi >= 0
        assert c.admit[density][gi[real]].all(), density  # admitted rows only
        if density == 'none':
            assert (gi == -1).all() and (gbits == 0x7f800000).all()
        if density == 'one':
            assert (real.sum(1) <= 1).all() and real[:, 0].all()  # (the one admitted row is a seed: every query lists it, first)


SHAPES = [(128, 32, 128, 64), (64, 32, 64, 64), (3, 5, 10, 10), (200, 17, 33, 7), (128, 32, 200, 129), (768, 24, 256, 256),
          (128, 64, 100, 1)]
CASES = [(EUCLIDEAN, *s) for s in SHAPES] + [(m, *s) for m in (INNER_PRODUCT, COSINE) for s in SHAPES[:2]]


@pytest.mark.parametrize('metric,D,L,ef_route,ef', CASES)
def test_filtered_walk_equals_its_restatement(ops, metric, D, L, ef_route, ef):
    c = _case(ops, metric, D, L)
    if metric == INNER_PRODUCT:
        assert (c.dist[0] < 0).sum() > N // 10  # negative distances: the key, not the float's bits, orders them
    if metric == EUCLIDEAN:
        assert c.dist[c.self_q, c.self_row] == 0.0
    _assert_equals_restated(ops, c, ef_route, ef)
    if metric == EUCLIDEAN:
        gi, gbits = _run(ops, c, ef_route, ef, 'one')
        assert gi[c.self_q, 0] == c.self_row and gbits[c.self_q, 0] == 0  # the stored row finds itself at +0.0


@pytest.mark.parametrize('metric,D,L,ef_route', [(EUCLIDEAN, 128, 32, 128), (EUCLIDEAN, 3, 5, 10), (COSINE, 64, 32, 64)])
def test_all_rows_admitted_at_ef_route_is_the_plain_walk(ops, metric, D, L, ef_route):
    """ef = ef_route, every row admitted: the result list is annlite_graph_f32_search's list."""
    import torch

    c = _case(ops, metric, D, L)
    gi, gbits = _run(ops, c, ef_route, ef_route, 'all')
    pi, pd = ops.graph_f32_search(metric, c.q_d, c.x_d, c.links_d, c.seeds_d, ef_route)
    torch.cuda.synchronize()
    assert np.array_equal(gi, pi.cpu().numpy()) and np.array_equal(gbits, pd.cpu().numpy().view(np.uint32))


# (registers per lane of the routing and of the result list: (1, 1), (2, 1), (2, 2), (4, 4), (4, 2), (4, 1))
SMALL_TABLE = [(EUCLIDEAN, 128, 32, 64, 64), (EUCLIDEAN, 128, 32, 128, 64), (EUCLIDEAN, 128, 32, 128, 100), (EUCLIDEAN, 128, 32, 256, 129),
               (INNER_PRODUCT, 64, 32, 200, 100), (COSINE, 64, 32, 256, 10)]


@pytest.mark.parametrize('hash_bits', [4, 6])
@pytest.mark.parametrize('metric,D,L,ef_route,ef', SMALL_TABLE)
def test_a_full_visited_table_changes_nothing_in_the_result_list(ops, monkeypatch, metric, D, L, ef_route, ef, hash_bits):
    """ANNLITE_GRAPH_HASH_BITS = 4 / 6 (16 / 64 visited entries): every neighbour is reported as new, evaluated again and offered to
    both lists again.  The result list is the default table's and the restatement's, no id twice; the counters show that the path ran:
    the expansions of the plain walk at ``ef_route``, more rows evaluated."""
    import torch

    c = _case(ops, metric, D, L)
    default = {density: _run(ops, c, ef_route, ef, density) for density in ('0.5', 'all')}
    monkeypatch.setenv('ANNLITE_GRAPH_HASH_BITS', str(hash_bits))
    for density in ('0.5', 'all'):
        wi, wbits, _ = _restated(c, ef_route, ef, density)
        gi, gbits = _run(ops, c, ef_route, ef, density)
        for b in range(c.b):
            assert np.array_equal(gi[b], wi[b]) and np.array_equal(gbits[b], wbits[b]), (density, b)
            real = gi[b][gi[b] >= 0]
            assert np.unique(real).size == real.size
        assert np.array_equal(gi, default[density][0]) and np.array_equal(gbits, default[density][1]), density
    monkeypatch.setenv('ANNLITE_DEBUG_COUNTERS', '1')
    _run(ops, c, ef_route, ef, '0.5')
    small = ops.graph_f32_search_stats()
    monkeypatch.delenv('ANNLITE_GRAPH_HASH_BITS')
    _run(ops, c, ef_route, ef, '0.5')
    large = ops.graph_f32_search_stats()
    ops.graph_f32_search(metric, c.q_d, c.x_d, c.links_d, c.seeds_d, ef_route)
    torch.cuda.synchronize()
    plain = ops.graph_f32_search_stats()
    tot = _restated(c, ef_route, ef, '0.5')[2]
    print(f'hash_bits={hash_bits} (expansions, rows): small table {small}, default table {large}, plain walk {plain}, restated {tot}')
    assert small[0] == large[0] == plain[0] == tot['expansions']
    assert large[1] == plain[1] == tot['evals']
    assert small[1] > large[1]


def test_the_filter_does_not_route(ops, monkeypatch):
    """Expansions and rows evaluated are the plain walk's at ``ef_route`` under every filter."""
    import torch

    c = _case(ops, EUCLIDEAN, 128, 32)
    monkeypatch.setenv('ANNLITE_DEBUG_COUNTERS', '1')
    ops.graph_f32_search(EUCLIDEAN, c.q_d, c.x_d, c.links_d, c.seeds_d, 128)
    torch.cuda.synchronize()
    plain = ops.graph_f32_search_stats()
    lk = c.links.view(np.uint32)
    tot = [0, 0]
    for b in range(c.b):
        st = {}
        walk_restated(lk, c.seeds, c.keys[b], 128, stats=st)
        tot = [tot[0] + st['expansions'], tot[1] + st['evals']]
    assert list(plain) == tot
    for density in DENSITIES:
        _run(ops, c, 128, 64, density)
        assert ops.graph_f32_search_stats() == plain, density


@pytest.mark.parametrize('D,L,ef_route,ef', [(1, 8, 16, 5), (16, 8, 1, 1), (16, 1, 10, 10)])
def test_filtered_walk_at_one_dimension_one_entry_one_link(ops, D, L, ef_route, ef):
    _assert_equals_restated(ops, _case(ops, EUCLIDEAN, D, L), ef_route, ef)


@pytest.mark.parametrize('metric,ef_route,ef', [(EUCLIDEAN, 64, 64), (INNER_PRODUCT, 256, 100)])
def test_filtered_walk_at_2048_dimensions(ops, metric, ef_route, ef):
    """8 KB of query per wave: workgroups of three waves, ten queries leave the last one wave."""
    _assert_equals_restated(ops, _case(ops, metric, 2048, 16, n=600), ef_route, ef, ('0.5', 'one', 'none'))


def test_filtered_walk_with_one_query(ops):
    _assert_equals_restated(ops, _case(ops, EUCLIDEAN, 128, 32, b=1), 128, 64)


@pytest.mark.parametrize('seeds', ['1', '65', 'beyond'])
def test_filtered_walk_seed_sets(ops, seeds):
    c = _case(ops, EUCLIDEAN, 128, 32, seeds=seeds)
    if seeds == 'beyond':
        assert (c.seeds.astype(np.int64) >= c.n).sum() == N_SEEDS // 5
    _assert_equals_restated(ops, c, 128, 64)
    gi, _ = _run(ops, c, 128, 64, '0.5')
    assert (gi >= 0).sum(1).min() == 64  # (the walk went somewhere: a full list of admitted rows)


@pytest.mark.parametrize('admitted', [True, False])
def test_filtered_walk_over_one_row(ops, admitted):
    import torch

    x = np.array([[1.0, 2.0, 3.0]], np.float32)
    q = np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 1.0]], np.float32)
    links = np.zeros((1, 9), np.int32)
    seeds = np.zeros(1, np.int32)
    admit = np.array([admitted])
    gi, gd = ops.graph_f32_search_admit(EUCLIDEAN, ops.to_dev(q), ops.to_dev(x), ops.to_dev(links), ops.to_dev(seeds), 10, 4,
                                        ops.to_dev(bitmap(admit)))
    torch.cuda.synchronize()
    gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
    first = 0 if admitted else -1
    assert np.array_equal(gi, np.array([[first, -1, -1, -1]] * 2))
    inf = np.inf
    assert np.array_equal(gd, np.array([[0.0 if admitted else inf, inf, inf, inf], [9.0 if admitted else inf, inf, inf, inf]], np.float32))
    keys = f32_key(np.array([[0.0], [9.0]], np.float32))
    for b in range(2):
        ri, rbits = walk_admit_restated(links.view(np.uint32), seeds, keys[b], 10, 4, admit)
        assert np.array_equal(gi[b], ri) and np.array_equal(gd[b].view(np.uint32), rbits)


def test_filtered_walk_over_no_row(ops):
    """N = 0 (storage allocated, nothing written): no seed is a row, every output is (-1, +inf)."""
    import torch

    c = _case(ops, EUCLIDEAN, 128, 32)
    gi, gd = ops.graph_f32_search_admit(EUCLIDEAN, c.q_d, c.x_d, c.links_d, c.seeds_d, 64, 10, c.admit_d['all'], n_rows=0)
    torch.cuda.synchronize()
    assert (gi.cpu().numpy() == -1).all() and np.isposinf(gd.cpu().numpy()).all()


def test_filtered_walk_refuses_what_it_cannot_hold(ops):
    """ef > ef_route, ef_route beyond 256, D beyond 2048 and a missing bitmap are refused by the library's parameter checks: nothing
    is launched (the outputs of a launch would need the bitmap)."""
    import torch

    rs = np.random.RandomState(1)
    links = ops.to_dev(random_links(rs, 100, 8))
    seeds = ops.to_dev(np.arange(10, dtype=np.int32))
    admit = ops.to_dev(bitmap(np.ones(100, bool)))
    x = torch.zeros((100, 8), dtype=torch.float32, device='cuda')
    with pytest.raises(Exception, match='ef_route'):
        ops.graph_f32_search_admit(EUCLIDEAN, x[:2].contiguous(), x, links, seeds, 16, 17, admit)
    with pytest.raises(Exception, match='ef_route'):
        ops.graph_f32_search_admit(EUCLIDEAN, x[:2].contiguous(), x, links, seeds, 257, 16, admit)
    with pytest.raises(Exception, match='admit_bits'):
        ops.graph_f32_search_admit(EUCLIDEAN, x[:2].contiguous(), x, links, seeds, 16, 16, None)
    x = torch.zeros((100, 2049), dtype=torch.float32, device='cuda')
    with pytest.raises(Exception, match='2048'):
        ops.graph_f32_search_admit(EUCLIDEAN, x[:2].contiguous(), x, links, seeds, 16, 16, admit)
    torch.cuda.synchronize()
