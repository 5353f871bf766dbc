"""The float graph walk (annlite_graph_f32_search, graph_f32.hip) pinned BIT FOR BIT against a plain restatement of its order.

The order is that of the PQ walk one node at a time (tests/test_graph_pair.py ``walk_restated`` with width 1, restated in
tests/_refs.py): seeds scanned flat in rounds of 64, the best unexpanded entry expanded, a step's unseen neighbours (ids < N) tested
against the list's worst entry BEFORE any of them is inserted, the walk over when the first min(ef, 64 E) entries hold no unexpanded
node.  What differs is the distance: ``ops.exact_gather_dist`` over all rows is the oracle -- the kernel's distances carry its bits --
and the list is ordered by (``f32_key(distance)``, node id): negative distances (INNER_PRODUCT) ascend, NaN sorts behind +inf.

Beyond the comfortable shapes: a visited table of 16 or 64 entries (every node evaluated again and again, the merge's duplicate
check alone keeps the list right: tests/test_graph_f32_restated.py is the argument, without a GPU), D = 1 and D = 2048 (three waves
per workgroup), ef = 1, L = 1, B = 1, one seed, 64 and 65 seeds, seeds beyond the table, a table of one row -- and the returned
distances against float64 within the fp32 summation bound of tests/test_rerank_topk.py."""
import numpy as np
import pytest

from _refs import bitmap, f32_key, fp32_chain_bound, random_links as _random_graph, walk_restated
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

EUCLIDEAN, INNER_PRODUCT, COSINE = 1, 2, 3
N, B, N_SEEDS = 3000, 10, 150


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


SHAPES = [(128, 32, 128), (64, 32, 64), (3, 5, 10), (200, 17, 33), (128, 32, 129), (128, 32, 200), (768, 24, 256), (128, 64, 100)]
CASES = [(EUCLIDEAN, *s) for s in SHAPES] + [(m, *s) for m in (INNER_PRODUCT, COSINE) for s in SHAPES[:2]]


@pytest.mark.parametrize('metric,D,L,ef', CASES)
def test_float_walk_equals_its_restatement(ops, metric, D, L, ef):
    import torch

    rs = np.random.RandomState(metric * 100003 + D * 1000 + L * 7 + ef)
    links = _random_graph(rs, N, L)
    x = rs.randn(N, D).astype(np.float32)
    x[1000:1040] = x[1000]  # exact ties inside the walk: the key's low word (the node id) decides
    q = rs.randn(B, D).astype(np.float32)
    q[2] = x[77]  # a stored row as its own query
    if metric == COSINE:  # (the index stores and asks normalised rows; the kernel computes 1 - <q, x> on what it is given)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[4, D // 2] = np.nan
    q[7, 0] = np.inf
    seeds = rs.choice(N, N_SEEDS, replace=False).astype(np.int32)  # three rounds of 64, the last one partial
    valid = rs.rand(N) < 0.9
    x_d, q_d, links_d, seeds_d = ops.to_dev(x), ops.to_dev(q), ops.to_dev(links), ops.to_dev(seeds)
    vb = ops.to_dev(bitmap(valid))
    all_rows = torch.arange(N, device='cuda', dtype=torch.int64)[None, :].expand(B, N).contiguous()
    dist = ops.exact_gather_dist(metric, q_d, x_d, all_rows).cpu().numpy()  # the oracle: the bits every kernel distance carries
    if metric == INNER_PRODUCT:
        assert (dist[0] < 0).sum() > N // 10  # negative distances: the key, not the float's bits, orders them
    if metric == EUCLIDEAN:
        assert dist[2, 77] == 0.0
    assert np.isnan(dist[4]).all() and not np.isfinite(dist[7]).any()
    keys = f32_key(dist)
    lk = links.view(np.uint32)
    for vbits, vmask in ((None, None), (vb, valid)):
        gi, gd = ops.graph_f32_search(metric, q_d, x_d, links_d, seeds_d, ef, valid_bits=vbits)
        torch.cuda.synchronize()
        gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
        for b in range(B):
            ri, rbits = walk_restated(lk, seeds, keys[b], ef, vmask)
            assert np.array_equal(gi[b], ri), (vmask is not None, b)
            assert np.array_equal(gd[b].view(np.uint32), rbits), (vmask is not None, b)


def test_float_walk_refuses_what_it_cannot_hold(ops):
    import torch

    rs = np.random.RandomState(1)
    links = ops.to_dev(_random_graph(rs, 100, 8))
    seeds = ops.to_dev(np.arange(10, dtype=np.int32))
    x = torch.zeros((100, 2049), dtype=torch.float32, device='cuda')
    with pytest.raises(Exception, match='2048'):
        ops.graph_f32_search(EUCLIDEAN, x[:2].contiguous(), x, links, seeds, 16)
    x = torch.zeros((100, 8), dtype=torch.float32, device='cuda')
    with pytest.raises(Exception, match='ef'):
        ops.graph_f32_search(EUCLIDEAN, x[:2].contiguous(), x, links, seeds, 257)


# ---- the same data at any size, made once per shape and shared: the tests below leave it unchanged ------------------------------
class _Case:
    pass


_cases = {}


def _case(ops, metric, D, L, n=N, b=B, seeds='150'):
    """The data of the test above for a table of ``n`` rows and ``b`` queries: tie block, a stored row as its own query, a NaN and an
    inf query (where the batch has them), a neighbour listed twice, ids beyond the table; the distance matrix of
    ``exact_gather_dist`` and its keys.  ``seeds``: '150' distinct ids, '1' / '64' / '65' of them, or 'beyond': every fifth id >= n."""
    import torch

    key = (metric, D, L, n, b, seeds)
    if key in _cases:
        return _cases[key]
    rs = np.random.RandomState(metric * 100003 + D * 1000 + L * 7 + n + 31 * b)
    c = _Case()
    c.metric, c.D, c.L, c.n, c.b = metric, D, L, n, b
    c.links = _random_graph(rs, n, L)
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
    full = np.nonzero(c.links.view(np.uint32)[:, 0] == L)[0]  # (seeds with a full list: a walk from one seed goes somewhere)
    n_seeds = N_SEEDS if seeds in ('150', 'beyond') else int(seeds)
    c.seeds = rs.choice(full, n_seeds, replace=False).astype(np.int64)
    if n_seeds >= 64 and c.self_row not in c.seeds:
        c.seeds[1] = c.self_row  # (the links are random, not a proximity graph: the row that is its own query is a seed)
    if seeds == 'beyond':
        c.seeds[::5] = n + np.arange(c.seeds[::5].size) * 7  # skipped: neither evaluated nor recorded
        c.seeds[5] = 0xfffffffe  # (the largest id the format has)
    c.seeds = c.seeds.astype(np.uint32)
    c.valid = rs.rand(n) < 0.9
    c.x_d, c.q_d, c.links_d, c.seeds_d = ops.to_dev(c.x), ops.to_dev(c.q), ops.to_dev(c.links), ops.to_dev(c.seeds)
    c.vb = ops.to_dev(bitmap(c.valid))
    all_rows = torch.arange(n, device='cuda', dtype=torch.int64)[None, :].expand(b, n).contiguous()
    c.dist = ops.exact_gather_dist(metric, c.q_d, c.x_d, all_rows).cpu().numpy()
    if b > 7:
        assert np.isnan(c.dist[4]).all() and not np.isfinite(c.dist[7]).any()
    c.keys = f32_key(c.dist)
    c.restated = {}
    _cases[key] = c
    return c


def _restated(c, ef):
    """{masked: ([ids per query], [bits per query])} and the walk's counters summed over the batch, computed once per (case, ef)"""
    if ef not in c.restated:
        lk = c.links.view(np.uint32)
        out = {}
        tot = dict(expansions=0, evals=0)
        for masked in (False, True):
            rows = []
            for b in range(c.b):
                st = {}
                rows.append(walk_restated(lk, c.seeds, c.keys[b], ef, c.valid if masked else None, stats=st))
                if not masked:
                    tot = {k: tot[k] + st[k] for k in tot}
            out[masked] = (np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]))
        c.restated[ef] = (out, tot)
    return c.restated[ef]


def _run(ops, c, ef, masked):
    import torch

    gi, gd = ops.graph_f32_search(c.metric, c.q_d, c.x_d, c.links_d, c.seeds_d, ef, valid_bits=c.vb if masked else None)
    torch.cuda.synchronize()
    return gi.cpu().numpy(), gd.cpu().numpy().view(np.uint32)


def _assert_equals_restated(ops, c, ef):
    want, _ = _restated(c, ef)
    for masked in (False, True):
        gi, gbits = _run(ops, c, ef, masked)
        for b in range(c.b):
            assert np.array_equal(gi[b], want[masked][0][b]), (masked, b)
            assert np.array_equal(gbits[b], want[masked][1][b]), (masked, b)


FULL_TABLE = [(EUCLIDEAN, 128, 32, 64), (EUCLIDEAN, 128, 32, 128), (EUCLIDEAN, 128, 32, 256), (EUCLIDEAN, 128, 64, 100),
              (INNER_PRODUCT, 64, 32, 200), (COSINE, 64, 32, 64)]


@pytest.mark.parametrize('hash_bits', [4, 6])
@pytest.mark.parametrize('metric,D,L,ef', FULL_TABLE)
def test_a_full_visited_table_changes_nothing_but_the_rows_evaluated(ops, monkeypatch, metric, D, L, ef, hash_bits):
    """ANNLITE_GRAPH_HASH_BITS = 4 / 6: 16 / 64 visited entries against lists of 64 .. 256 -- Beam::visit gives up from the seeds
    on (16 probes: four times round the four buckets of the 16-entry table), every neighbour is reported as new and evaluated again,
    and the merge's ``tbl_full`` branch has to see the duplicate and take the careful path (E = 1, 2 and 4).  The list is the
    restatement's and the default table's, bit for bit; the counters show that the path ran: as many expansions, more rows."""
    c = _case(ops, metric, D, L)
    want, tot = _restated(c, ef)
    default = {masked: _run(ops, c, ef, masked) for masked in (False, True)}
    monkeypatch.setenv('ANNLITE_GRAPH_HASH_BITS', str(hash_bits))
    for masked in (False, True):
        gi, gbits = _run(ops, c, ef, masked)
        for b in range(c.b):
            assert np.array_equal(gi[b], want[masked][0][b]), (masked, b)
            assert np.array_equal(gbits[b], want[masked][1][b]), (masked, b)
            real = gi[b][gi[b] >= 0]
            assert np.unique(real).size == real.size  # no node twice in a list
        assert np.array_equal(gi, default[masked][0]) and np.array_equal(gbits, default[masked][1]), masked
    monkeypatch.setenv('ANNLITE_DEBUG_COUNTERS', '1')
    _run(ops, c, ef, False)
    small = ops.graph_f32_search_stats()
    monkeypatch.delenv('ANNLITE_GRAPH_HASH_BITS')
    _run(ops, c, ef, False)
    large = ops.graph_f32_search_stats()
    print(f'hash_bits={hash_bits} (expansions, rows): small table {small}, default table {large}, restated {tot}')
    assert small[0] == large[0] == tot['expansions']
    assert large[1] == tot['evals']  # (the default table held every node: each row once)
    assert small[1] > large[1]


def _extreme(ops, metric, D, L, ef, **kw):
    _assert_equals_restated(ops, _case(ops, metric, D, L, **kw), ef)


@pytest.mark.parametrize('D,L,ef', [(1, 8, 16), (16, 8, 1), (16, 1, 10)])
def test_float_walk_at_one_dimension_one_entry_one_link(ops, D, L, ef):
    _extreme(ops, EUCLIDEAN, D, L, ef)


@pytest.mark.parametrize('metric', [EUCLIDEAN, INNER_PRODUCT])
@pytest.mark.parametrize('ef', [64, 256])
def test_float_walk_at_2048_dimensions(ops, metric, ef):
    """8 KB of query per wave: workgroups of three waves (192 threads), ten queries leave the last one wave."""
    _extreme(ops, metric, 2048, 16, ef, n=600)


@pytest.mark.parametrize('b', [1, 5])
def test_float_walk_with_few_queries(ops, b):
    _extreme(ops, EUCLIDEAN, 128, 32, 128, b=b)


@pytest.mark.parametrize('seeds', ['1', '64', '65', 'beyond'])
def test_float_walk_seed_sets(ops, seeds):
    """One seed, exactly one round, one round and one id, and a set in which every fifth id is not a row (skipped)."""
    c = _case(ops, EUCLIDEAN, 128, 32, seeds=seeds)
    if seeds == 'beyond':
        assert (c.seeds.astype(np.int64) >= c.n).sum() == N_SEEDS // 5
    _assert_equals_restated(ops, c, 128)
    gi, _ = _run(ops, c, 128, False)
    assert (gi >= 0).sum(1).min() > 64  # (the walk went somewhere: more entries than one round of seeds)


def test_float_walk_over_one_row(ops):
    """N = 1: one node without links, seeds [0]: one real entry, then (-1, +inf)."""
    import torch

    x = np.array([[1.0, 2.0, 3.0]], np.float32)
    q = np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 1.0]], np.float32)
    links = np.zeros((1, 9), np.int32)
    links[0, 1:] = 0  # (slots beyond the count: never read as neighbours)
    seeds = np.zeros(1, np.int32)
    gi, gd = ops.graph_f32_search(EUCLIDEAN, ops.to_dev(q), ops.to_dev(x), ops.to_dev(links), ops.to_dev(seeds), 10)
    torch.cuda.synchronize()
    gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
    assert np.array_equal(gi, np.array([[0] + [-1] * 9] * 2))
    assert np.array_equal(gd, np.array([[0.0] + [np.inf] * 9, [9.0] + [np.inf] * 9], np.float32))
    keys = f32_key(np.array([[0.0], [9.0]], np.float32))
    for b in range(2):
        ri, rbits = walk_restated(links.view(np.uint32), seeds, keys[b], 10)
        assert np.array_equal(gi[b], ri) and np.array_equal(gd[b].view(np.uint32), rbits)


@pytest.mark.parametrize('metric', [EUCLIDEAN, INNER_PRODUCT, COSINE])
@pytest.mark.parametrize('D', [1, 768, 2048])
def test_float_walk_distances_against_float64(ops, metric, D):
    """Every finite (id, distance) the walk returns lies within the fp32 summation bound of the float64 distance of that row
    (``_refs.fp32_chain_bound``: the chain of annlite_exact_gather_dist, which the tests above take as the oracle); a stored row
    asked for itself is found at exactly 0.0 (EUCLIDEAN)."""
    c = _case(ops, metric, D, 16, n=600 if D == 2048 else N)
    ef = 64
    _assert_equals_restated(ops, c, ef)
    gi, gbits = _run(ops, c, ef, False)
    gd = gbits.view(np.float32)
    checked = 0
    for b in range(c.b):
        ok = (gi[b] >= 0) & np.isfinite(gd[b])
        ids = gi[b][ok]
        x64, q64 = c.x[ids].astype(np.float64), c.q[b].astype(np.float64)
        terms = (x64 - q64) ** 2 if metric == EUCLIDEAN else x64 * q64
        d64 = terms.sum(1) if metric == EUCLIDEAN else 1.0 - terms.sum(1)
        tol = fp32_chain_bound(terms, d64, D)
        err = np.abs(gd[b][ok].astype(np.float64) - d64)
        assert (err <= tol).all(), (b, float((err / np.maximum(tol, 1e-300)).max()))
        checked += ids.size
    assert checked >= (c.b - 2) * ef  # (all but the NaN and the inf query returned finite distances)
    if metric == EUCLIDEAN:
        assert gi[c.self_q, 0] == c.self_row and gbits[c.self_q, 0] == 0  # +0.0
