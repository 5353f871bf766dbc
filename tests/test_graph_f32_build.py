"""The float graph's build kernels (annlite_graph_f32_build_select / annlite_graph_f32_build_reverse, graph_f32.hip) against plain
restatements of their rules -- those of tests/test_graph_gpu_build.py (hnsw_host.cpp select_neighbors / connect), restated here with
the float distance: every distance is read from an N x N matrix of ``ops.exact_gather_dist`` bits, the numbers the kernels compare."""
import numpy as np
import pytest

from _refs import f32_key
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]
SENT = np.iinfo(np.int64).max
EUCLIDEAN, INNER_PRODUCT, COSINE = 1, 2, 3
N = 3000


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


_cache = {}


BAD_ROWS = (-30, -25, -20, -12, -7)  # (of the `bad` table, from its end: inside a batch of its last 37 rows)


def _table(ops, D, metric, n=N, bad=False):
    """n clustered rows with near-duplicates and exact duplicates, and their n x n distance matrix (computed once per shape).
    ``bad``: five rows hold a NaN or a +inf coordinate."""
    import torch

    key = (D, metric) if (n, bad) == (N, False) else (D, metric, n, bad)
    if key not in _cache:
        rs = np.random.RandomState(D * 10 + metric)
        n_dup = 300 if n == N else n // 10
        centers = (2.0 * rs.randn(12, D)).astype(np.float32)
        x = (centers[rs.randint(0, 12, n)] + 0.3 * rs.randn(n, D)).astype(np.float32)
        near = rs.choice(n, n_dup, replace=False)
        x[near] = (x[rs.randint(0, n, n_dup)] * np.float32(1 + 2 ** -20)).astype(np.float32)  # near-duplicates
        dup = rs.choice(n, n_dup, replace=False)
        x[dup] = x[rs.randint(0, n, n_dup)]  # exact duplicates: distance 0 between candidates, ties
        if metric == COSINE:
            x /= np.linalg.norm(x, axis=1, keepdims=True)
        if bad:
            for j, r in enumerate(BAD_ROWS):
                x[n + r, (7 * j) % D] = np.nan if j % 2 == 0 else np.inf  # three NaN rows, two +inf rows
        x_d = ops.to_dev(x)
        rows = torch.arange(n, device='cuda', dtype=torch.int64)[None, :].expand(n, n).contiguous()
        dm = ops.exact_gather_dist(metric, x_d, x_d, rows).cpu().numpy()
        if bad:  # (a NaN's sign and payload are nobody's contract: the keys, which is what the kernels order by, are symmetric)
            assert np.array_equal(f32_key(dm), f32_key(dm.T.copy())) and np.isnan(dm).sum() > 3 * n and np.isinf(dm).sum() > n
        else:
            assert np.array_equal(dm.view(np.uint32), dm.T.copy().view(np.uint32))  # the arithmetic is symmetric, bit for bit
        _cache[key] = (x, x_d, dm)
    return _cache[key]


def _twins(x):
    """twin[r]: another row that holds exactly r's vector, or -1"""
    _, first, inv, cnt = np.unique(x, axis=0, return_index=True, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    last = np.zeros(first.size, np.int64)
    last[inv] = np.arange(x.shape[0])  # (the highest row of each group)
    twin = np.where(first[inv] != np.arange(x.shape[0]), first[inv], last[inv])
    return np.where(cnt[inv] > 1, twin, -1)


def _heuristic(dm, base, pool, m_max):
    """Algorithm 4 over rows in visiting order: a candidate is kept unless a kept neighbour is STRICTLY closer to it than the base
    point is (``not (d < tb)``: a NaN on either side keeps the candidate)."""
    keep = []
    for c in pool:
        if len(keep) >= m_max:
            break
        tb = dm[base, c]
        if all(not (dm[k, c] < tb) for k in keep):
            keep.append(c)
    return keep


def _select(dm, base, pool, m_max):
    """hnsw_host.cpp select_neighbors over a pool that is already in visiting order (holes, the point itself and ids that are no
    rows of the table skipped)."""
    pool = [int(p) for p in pool if 0 <= p < dm.shape[0] and p != base]
    if len(pool) <= m_max:
        return pool
    return _heuristic(dm, base, pool, m_max)


@pytest.mark.parametrize('metric,D,ef,keep', [(EUCLIDEAN, 32, 200, 16), (EUCLIDEAN, 100, 256, 12), (EUCLIDEAN, 32, 10, 16),
                                             (EUCLIDEAN, 100, 40, 4), (INNER_PRODUCT, 32, 200, 12), (COSINE, 100, 256, 16)])
def test_float_select_kernel_is_algorithm_4(ops, metric, D, ef, keep):
    import torch

    rs = np.random.RandomState(D + ef + metric)
    x, x_d, dm = _table(ops, D, metric)
    b = 37
    base0 = N - b
    cand = np.full((b, ef), -1, np.int64)
    for i in range(b):
        n_c = ef if i % 5 else rs.randint(0, ef + 1)  # ragged lists, some shorter than `keep`
        ids = rs.choice(base0, n_c, replace=False)
        # visiting order = the base point's distance, with a few holes and the point itself
        ids = ids[np.argsort(f32_key(dm[base0 + i, ids]), kind='stable')]
        cand[i, :n_c] = ids
        if n_c > 8:
            cand[i, rs.randint(0, n_c, 2)] = -1
            cand[i, rs.randint(0, n_c)] = base0 + i
    lpn = 32
    links = torch.zeros((N, lpn + 1), dtype=torch.int32, device='cuda')
    pairs = ops.graph_f32_build_select(metric, ops.to_dev(cand), base0, x_d, keep, links)
    torch.cuda.synchronize()
    lk, pr = links.cpu().numpy().view(np.uint32), pairs.cpu().numpy()
    pruned = 0
    for i in range(b):
        want = _select(dm, base0 + i, cand[i], keep)
        row = lk[base0 + i]
        assert int(row[0]) == len(want), (i, row[:8], want)
        assert row[1:1 + len(want)].tolist() == want, i
        got_pairs = [int(p) for p in pr[i] if p != SENT]
        assert got_pairs == [(t << 32) | (base0 + i) for t in want]
        real = [int(p) for p in cand[i] if p >= 0 and p != base0 + i]
        pruned += len(real) > keep and want != real[:keep]
    assert pruned > 0 or ef <= keep  # (the heuristic did reject candidates: the check is not the first-`keep` rule)
    assert not lk[:base0].any()  # nobody else's row is touched


@pytest.mark.parametrize('metric,D', [(EUCLIDEAN, 32), (EUCLIDEAN, 100), (INNER_PRODUCT, 32)])
def test_float_reverse_kernel_appends_dedupes_and_shrinks(ops, metric, D):
    import torch

    rs = np.random.RandomState(9 + D + metric)
    x, x_d, dm = _table(ops, D, metric)
    lpn, half = 32, 1000
    links = np.zeros((N, lpn + 1), np.uint32)
    links[:, 1:] = 7  # (slots beyond a count hold anything)
    targets = rs.choice(half, 120, replace=False)
    pairs = []
    want = {}
    shrunk = 0
    for t_i, t in enumerate(targets):
        c = [0, 5, 20, 31, 32, 32, 32][t_i % 7]
        cur = [int(v) for v in rs.choice(np.setdiff1d(np.arange(half), [t]), c, replace=False)]
        links[t, 0] = c
        links[t, 1:1 + c] = cur
        k = [1, 3, 12, 1, 1, 7, 40][(t_i // 7) % 7]
        src = [int(v) for v in rs.choice(np.arange(half, N), k, replace=False)]
        if cur and t_i % 3 == 0:
            src.append(cur[0])  # a source that is in the list already: dropped
        if t_i % 11 == 0:
            src.append(int(t))  # the target itself: dropped
        src = sorted(set(src))
        pairs += [(int(t) << 32) | s for s in src]
        pool = cur + [s for s in src[: 64 - c] if s not in cur and s != t]  # at most 64 - count sources are taken
        if len(pool) == len(cur):
            want[int(t)] = cur
        elif len(pool) <= lpn:
            want[int(t)] = pool
        else:
            kt = f32_key(dm[t])
            order = sorted(pool, key=lambda v: (int(kt[v]), v))
            want[int(t)] = _select(dm, int(t), order, lpn)
            shrunk += 1
    assert shrunk >= 20
    keys = np.array(sorted(pairs), dtype=np.int64)
    tg = keys >> 32
    bounds = np.concatenate([[0], np.nonzero(np.diff(tg))[0] + 1, [len(keys)]]).astype(np.int64)
    links_d = ops.to_dev(links.view(np.int32))
    ops.graph_f32_build_reverse(metric, ops.to_dev(keys), ops.to_dev(bounds), x_d, links_d)
    torch.cuda.synchronize()
    got = links_d.cpu().numpy().view(np.uint32)
    for t, w in want.items():
        assert int(got[t, 0]) == len(w), (t, got[t, :6], w[:6])
        assert got[t, 1:1 + len(w)].tolist() == w, t
    untouched = np.setdiff1d(np.arange(N), targets)
    assert np.array_equal(got[untouched], links[untouched])  # rows nobody links are untouched


# ---- away from links_per_node = 32 ----------------------------------------------------------------------------------------------
def _candidates(rs, dm, twin, base0, b, i, ef, extra=()):
    """One point's candidate list in visiting order, drawn from the WHOLE table: batch mates are ordinary candidates (the exact-list
    phase of the builder feeds them), a point's exact duplicate, where it has one, stands in its list, some entries are holes,
    the point itself, or no rows of the table at all (skipped)."""
    n = dm.shape[0]
    base = base0 + i
    n_c = ef if (i % 5 or b == 1) else rs.randint(0, ef + 1)  # ragged lists, some shorter than `keep`
    forced = [int(v) for v in extra if v != base]
    if twin[base] >= 0:
        forced.append(int(twin[base]))
    if b > 1:
        forced += [base0 + (i + 1) % b, base0 + (i + 7) % b]
    forced = list(dict.fromkeys(v for v in forced if v != base))[:n_c]
    rest = rs.choice(np.setdiff1d(np.arange(n), forced + [base]), n_c - len(forced), replace=False)
    ids = np.concatenate([np.array(forced, np.int64), rest.astype(np.int64)])
    ids = ids[np.argsort(f32_key(dm[base, ids]), kind='stable')]
    row = np.full(ef, -1, np.int64)
    row[:n_c] = ids
    if n_c > 8:
        row[rs.randint(1, n_c, 2)] = -1
        row[rs.randint(1, n_c)] = base
        if i % 3 == 0:
            row[rs.randint(1, n_c, 3)] = [n, n + 1 + i, (1 << 32) + int(ids[0])]  # (the last: a row's id in its low 32 bits)
    return row


def _check_select(ops, table, metric, ef, keep, lpn, b, base0, rs, extra=()):
    import torch

    x, x_d, dm = table
    n = dm.shape[0]
    twin = _twins(x)
    if b == 1 and base0 is None:
        # one point: one whose list the heuristic prunes, says the restatement -- with an exact duplicate in it if there is such a
        # point (keep = 2: there is none, the duplicate comes first and rejects nothing)
        tries = np.concatenate([np.nonzero(twin >= 0)[0][:40], np.nonzero(twin < 0)[0][:40]])
        for base0 in tries:
            cand = _candidates(rs, dm, twin, int(base0), 1, 0, ef, extra)[None, :]
            real = [int(p) for p in cand[0] if 0 <= p < n and p != base0]
            if _select(dm, int(base0), cand[0], keep) != real[:keep]:
                break
        else:
            raise AssertionError('no point with a pruned list among 80')
        base0 = int(base0)
    else:
        cand = np.stack([_candidates(rs, dm, twin, base0, b, i, ef, extra) for i in range(b)])
    links = torch.zeros((n, lpn + 1), dtype=torch.int32, device='cuda')
    pairs = ops.graph_f32_build_select(metric, ops.to_dev(cand), base0, x_d, keep, links)
    torch.cuda.synchronize()
    lk, pr = links.cpu().numpy().view(np.uint32), pairs.cpu().numpy()
    assert pr.shape == (b, keep)
    pruned = twin_kept = mates = beyond = 0
    for i in range(b):
        base = base0 + i
        want = _select(dm, base, cand[i], keep)
        row = lk[base]
        assert int(row[0]) == len(want), (i, row[:8], want)
        assert row[1:1 + len(want)].tolist() == want, i
        assert pr[i].tolist() == [(t << 32) | base for t in want] + [SENT] * (keep - len(want)), i
        real = [int(p) for p in cand[i] if 0 <= p < n and p != base]
        pruned += len(real) > keep and want != real[:keep]
        twin_kept += int(twin[base]) in want
        mates += sum(base0 <= p < base0 + b for p in want)
        beyond += int((cand[i] >= n).sum())
    assert pruned > 0 or ef <= keep  # (the heuristic did reject candidates: the check is not the first-`keep` rule)
    assert twin_kept > 0 or b == 1  # (a kept neighbour as far from every candidate as the point itself: `<`, not `<=`)
    assert beyond > 0 and (b == 1 or mates > 0)
    others = np.setdiff1d(np.arange(n), np.arange(base0, base0 + b))
    assert not lk[others].any()  # nobody else's row is touched
    return lk


SELECT_EDGES = [(EUCLIDEAN, 32, 256, 64, 64, N), (EUCLIDEAN, 100, 200, 2, 4, N), (EUCLIDEAN, 1, 40, 8, 16, N),
                (EUCLIDEAN, 2048, 64, 16, 32, 600), (COSINE, 768, 200, 16, 32, N), (INNER_PRODUCT, 100, 256, 16, 32, N)]


@pytest.mark.parametrize('b', [37, 1])
@pytest.mark.parametrize('metric,D,ef,keep,lpn,n', SELECT_EDGES)
def test_float_select_kernel_from_two_links_to_64_and_from_one_dimension_to_2048(ops, metric, D, ef, keep, lpn, n, b):
    rs = np.random.RandomState(D + ef + metric + 1000 * b)
    _check_select(ops, _table(ops, D, metric, n), metric, ef, keep, lpn, b, n - b if b > 1 else None, rs)


def test_float_select_kernel_on_the_first_rows_of_the_table(ops):
    rs = np.random.RandomState(4)
    _check_select(ops, _table(ops, 32, EUCLIDEAN), EUCLIDEAN, 200, 16, 32, 37, 0, rs)


def test_float_select_kernel_keeps_what_a_nan_cannot_reject(ops):
    """Five rows with a NaN or a +inf coordinate, base points of the batch and candidates of every list: ``not (d < tb)`` with a
    NaN on either side keeps the candidate (a NaN base point keeps its first `keep` candidates), a +inf base point rejects whatever
    stands at a finite distance from a kept neighbour."""
    n = 600
    x, x_d, dm = table = _table(ops, 32, EUCLIDEAN, n, bad=True)
    bad = [n + r for r in BAD_ROWS]
    rs = np.random.RandomState(5)
    lk = _check_select(ops, table, EUCLIDEAN, 64, 16, 32, 37, n - 37, rs, extra=bad)
    for r in bad:
        assert lk[r, 0] > 0
    assert sum(len(set(lk[i, 1:1 + lk[i, 0]].tolist()) & set(bad)) for i in range(n - 37, n)) > 0  # (they were kept, too)


def _reverse(dm, lpn, t, row, src):
    """connect()'s other half for one target: ``row`` its list (count, ids), ``src`` the ascending sources of its segment.  None: the
    row stays as it is.  The kernel's pool is 64 lanes: the first min(count, lpn) entries of the list, then as many sources as
    fit; of those, the target itself, ids that are no rows and ids the list holds are dropped.  With room the rest is appended; else
    the pool, ordered by (f32_key(distance to the target), id) -- a list entry that is no row of the table cannot be kept --, goes
    through Algorithm 4."""
    n = dm.shape[0]
    c = min(int(row[0]), lpn)
    cur = [int(v) for v in row[1:1 + c]]
    new = [int(s) for s in src[:64 - c] if s != t and s < n and s not in cur]
    if not new:
        return None
    pool = cur + new
    if len(pool) <= lpn:
        return pool
    kt = f32_key(dm[t])
    rows = sorted((v for v in pool if v < n), key=lambda v: (int(kt[v]), v))
    return _heuristic(dm, t, rows, lpn)


def _run_reverse(ops, metric, table, lpn, links, segs, n_rows=None):
    """``segs`` [(target, [sources])] (no sources: an empty segment) through the kernel on a copy of ``links``; every row compared
    with the restatement.  Returns how many rows were left alone, appended to and shrunk, and the lists after."""
    import torch

    x, x_d, dm = table
    n = dm.shape[0]
    segs = sorted(segs, key=lambda s: s[0])
    keys, bounds = [], [0]
    for t, src in segs:
        keys += [(int(t) << 32) | int(s) for s in sorted(set(src))]
        bounds.append(len(keys))
    assert keys == sorted(keys)
    links_d = ops.to_dev(links.view(np.int32).copy())
    ops.graph_f32_build_reverse(metric, ops.to_dev(np.array(keys, dtype=np.int64)), ops.to_dev(np.array(bounds, dtype=np.int64)), x_d, links_d)
    torch.cuda.synchronize()
    got = links_d.cpu().numpy().view(np.uint32)
    tally = dict(same=0, append=0, shrink=0)
    for t, src in segs:
        if t >= n:
            continue
        w = _reverse(dm, lpn, int(t), links[t], sorted(set(src)))
        if w is None:
            assert np.array_equal(got[t], links[t]), (t, got[t, :6], links[t, :6])
            tally['same'] += 1
            continue
        assert int(got[t, 0]) == len(w), (t, got[t, :6], w[:6])
        assert got[t, 1:1 + len(w)].tolist() == w, t
        tally['append' if _appended(dm, lpn, t, links[t], sorted(set(src))) else 'shrink'] += 1
    untouched = np.setdiff1d(np.arange(n), [t for t, _ in segs if t < n])
    assert np.array_equal(got[untouched], links[untouched])  # rows nobody links are untouched
    return tally, got


def _appended(dm, lpn, t, row, src):
    n = dm.shape[0]
    c = min(int(row[0]), lpn)
    cur = [int(v) for v in row[1:1 + c]]
    return c + len([s for s in src[:64 - c] if s != t and s < n and s not in cur]) <= lpn


@pytest.mark.parametrize('lpn', [1, 4, 16, 32])
@pytest.mark.parametrize('metric,D', [(EUCLIDEAN, 32), (COSINE, 100), (INNER_PRODUCT, 768)])
def test_float_reverse_kernel_at_every_list_length(ops, metric, D, lpn):
    """Lists of 0, lpn / 2, lpn - 1 and lpn entries, segments that bring nothing new, that fit and that do not (up to 70 sources:
    the pool takes 64 - count of them); a target's exact duplicate stands in its list or among its sources -- the neighbour that is
    as far from every candidate as the target itself, which `<` keeps from rejecting anything."""
    rs = np.random.RandomState(9 + D + metric + 100 * lpn)
    table = x, x_d, dm = _table(ops, D, metric)
    twin = _twins(x)
    half = 1000
    links = np.zeros((N, lpn + 1), np.uint32)
    links[:, 1:] = 7  # (slots beyond a count hold anything)
    with_twin = np.nonzero(twin[:half] >= 0)[0]
    targets = np.concatenate([with_twin[:48], rs.choice(np.setdiff1d(np.arange(half), with_twin[:48]), 132, replace=False)])
    segs = []
    twin_in_shrunk = 0
    for t_i, t in enumerate(targets):
        t = int(t)
        c = [0, lpn // 2, lpn - 1, lpn][t_i % 4]
        mode = ('append', 'same', 'shrink')[(t_i // 4) % 3]
        tw = int(twin[t]) if t_i < 48 else -1
        cur = [int(v) for v in rs.choice(np.setdiff1d(np.arange(half), [t, tw]), c, replace=False)]
        if tw >= 0 and c:
            cur[rs.randint(0, c)] = tw
        links[t, 0] = c
        links[t, 1:1 + c] = cur
        if mode == 'same':
            src = cur[::2] + ([t] if t_i % 2 else []) + ([N + t_i] if t_i % 3 == 0 or not c else [])
        else:
            room = lpn - c
            k = max(1, rs.randint(1, room + 1) if room else 1) if mode == 'append' else room + [1, 3, 40, 70][(t_i // 12) % 4]
            src = [int(v) for v in rs.choice(np.arange(half, N), k, replace=False)]
            if tw >= 0 and not c:
                src.append(tw)
            if cur and t_i % 3 == 0:
                src.append(cur[0])  # a source that is in the list already: dropped
            if t_i % 11 == 0:
                src.append(t)  # the target itself: dropped
        segs.append((t, src))
        w = _reverse(dm, lpn, t, links[t], sorted(set(src)))
        twin_in_shrunk += w is not None and tw >= 0 and tw in w and not _appended(dm, lpn, t, links[t], sorted(set(src)))
    tally, _ = _run_reverse(ops, metric, table, lpn, links, segs)
    assert min(tally.values()) >= 10, tally
    assert twin_in_shrunk >= 3


def test_float_reverse_kernel_on_lists_and_segments_no_builder_writes(ops):
    """A stored count above lpn (the first lpn entries are the list), list entries and sources that are no rows of the table, a
    target that is none, an empty segment -- and one and five segments: a workgroup with idle waves."""
    metric, lpn = EUCLIDEAN, 16
    table = x, x_d, dm = _table(ops, 32, metric)
    rs = np.random.RandomState(3)
    links = np.zeros((N, lpn + 1), np.uint32)
    links[:, 1:] = 7
    far = np.arange(1000, N)

    def fill(t, c, stored=None):
        links[t, 1:1 + c] = rs.choice(np.setdiff1d(np.arange(1000), [t]), c, replace=False)
        links[t, 0] = c if stored is None else stored
        return links[t, 1:1 + c].tolist()

    segs = []
    cur = fill(10, lpn, stored=lpn + 5)
    segs.append((10, cur[3:9] + [10]))  # nothing new: the row stays, count and all
    fill(20, lpn)
    links[20, 4] = N + 2  # a full list with an entry that is no row: the list shrinks, the entry goes
    segs.append((20, rs.choice(far, 3, replace=False).tolist()))
    fill(30, lpn // 2)
    links[30, 2] = N  # the same with room: the entry stays where it is
    segs.append((30, rs.choice(far, 2, replace=False).tolist()))
    fill(40, lpn // 2)
    segs.append((40, rs.choice(far, 2, replace=False).tolist() + [N, N + 9, 0xfffffffe]))  # sources that are no rows: dropped
    segs.append((50, []))  # an empty segment
    fill(50, 3)
    fill(60, lpn, stored=lpn + 1)  # (a count above lpn and something new: lpn entries and the sources, shrunk)
    segs.append((60, rs.choice(far, 4, replace=False).tolist()))
    segs.append((N + 3, [5, 6]))  # a target that is no row: nothing is written
    tally, got = _run_reverse(ops, metric, table, lpn, links, segs)
    assert tally == dict(same=2, append=2, shrink=2), tally  # (the empty segment counts as a row left alone)
    assert got[20, 0] <= lpn and N + 2 not in got[20, 1:1 + got[20, 0]]
    assert got[30, 0] == lpn // 2 + 2 and got[30, 2] == N
    assert got[40, 0] == lpn // 2 + 2
    assert np.array_equal(got[50], links[50])
    assert _run_reverse(ops, metric, table, lpn, links, segs[1:2])[0] == dict(same=0, append=0, shrink=1)  # S = 1
    assert _run_reverse(ops, metric, table, lpn, links, segs[:5])[0] == dict(same=2, append=2, shrink=1)  # S = 5


def test_float_reverse_kernel_orders_nan_behind_inf(ops):
    """Three NaN rows and two +inf rows as targets, in lists and among sources: the shrinking pool is ordered by ``f32_key`` -- NaN
    behind +inf, ties by id --, and a NaN distance rejects nothing."""
    metric, lpn, n = EUCLIDEAN, 16, 600
    table = x, x_d, dm = _table(ops, 32, metric, n, bad=True)
    bad = [n + r for r in BAD_ROWS]
    rs = np.random.RandomState(6)
    links = np.zeros((n, lpn + 1), np.uint32)
    segs = []
    for t_i, t in enumerate(bad + [3, 14, 15, 92, 65, 35]):
        c = lpn if t_i % 2 == 0 else lpn - 2
        pick = rs.choice(np.setdiff1d(np.arange(300), [t]), c, replace=False).tolist()
        others = [b for b in bad if b != t]
        pick[1], pick[5] = others[0], others[1]  # a NaN / inf row in the list ...
        links[t, 0] = c
        links[t, 1:1 + c] = pick
        src = rs.choice(np.arange(300, n - 40), 6, replace=False).tolist() + others[2:]  # ... and among the sources
        segs.append((t, src))
    tally, got = _run_reverse(ops, metric, table, lpn, links, segs)
    assert tally == dict(same=0, append=0, shrink=len(segs)), tally
    kept_bad = sum(len(set(got[t, 1:1 + got[t, 0]].tolist()) & set(bad)) for t, _ in segs)
    assert kept_bad > 0  # (rows at a NaN distance did come through)
