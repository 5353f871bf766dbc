"""numpy references shared by the kernel test files (not a conftest, no pytest setting): the NaN-last order with ties by id,
the oracle's top-k over arbitrary (distance, id) pairs, the SKEWED code layout, the key of a float, the validity bitmap, the float
graph walk's restatements and the fp32 summation bound of the exact distance.  Each is itself checked without a GPU, against the
oracle, a brute-force loop or a second statement, in tests/test_post_scan_kernels.py, tests/test_ivf_stage_kernels.py and
tests/test_graph_f32_restated.py."""
import numpy as np
import pytest

from conftest import has_gpu

gpu = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs an AMD GPU')]


def on_gpu(f):
    for m in gpu:
        f = m(f)
    return f


def bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


NANS = bits(0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffc12345)  # both signs, quiet / signalling, payloads
SUBNORMALS = bits(0x00000001, 0x80000001, 0x007fffff, 0x807fffff)


def lexsort_nan_last(vals, ids):
    """Permutation that sorts (vals, ids) ascending in numpy's order with ties by id: numbers by value (-0.0 == +0.0), then
    every NaN, each group by id."""
    vals = np.asarray(vals, dtype=np.float32)
    nan = np.isnan(vals)
    return np.lexsort((np.asarray(ids), np.where(nan, np.float32(0), vals), nan))


def topk_pairs(oracle, vals, ids, k):
    """The oracle's top-k over (distance, id) pairs with arbitrary distinct ids: pairs put in id order, so that the oracle's
    tie-break (position) IS the id.  Returns (f32 [k], i64 [k]) padded with (+inf, -1)."""
    vals, ids = np.asarray(vals, dtype=np.float32), np.asarray(ids, dtype=np.int64)
    by_id = np.argsort(ids, kind='stable')
    d, pos = oracle.top_k_c(vals[by_id], k)
    return d, np.where(pos >= 0, ids[by_id][np.clip(pos, 0, max(ids.size - 1, 0))] if ids.size else -1, -1)


def topk_pairs_numpy(vals, ids, k):
    """The same through the NaN-last lexsort (second, independent statement)."""
    vals, ids = np.asarray(vals, dtype=np.float32), np.asarray(ids, dtype=np.int64)
    o = lexsort_nan_last(vals, ids)[:k]
    pad = k - o.size
    return (np.concatenate([vals[o], np.full(pad, np.inf, np.float32)]), np.concatenate([ids[o], np.full(pad, -1, np.int64)]))


def skew_rows(plain, ids, inverse=False):
    """SKEWED storage of PLAIN rows: byte j of row n = code of sub-space (j + n) mod M; M = 64: two 32-byte
    halves, each rotated by n mod 32, and a byte whose position p = j mod 32 has p + n mod 32 >= 32 stores code - 1 (mod 256).
    ``inverse``: ``plain`` holds stored rows, the PLAIN rows come back."""
    plain = np.asarray(plain, dtype=np.uint8)
    ids = np.asarray(ids, dtype=np.int64)
    M = plain.shape[1]
    j = np.arange(M)[None, :]
    if M == 64:
        r = (ids % 32)[:, None]
        h, p = j // 32, j % 32
        if not inverse:
            src = 32 * h + (p + r) % 32
            return (np.take_along_axis(plain, src, axis=1).astype(np.int64) - (p + r >= 32)).astype(np.uint8)
        ps = (p - r) % 32                           # stored position (inside its half) of sub-space j
        return (np.take_along_axis(plain, 32 * h + ps, axis=1).astype(np.int64) + (ps + r >= 32)).astype(np.uint8)
    r = (ids % M)[:, None]
    return np.take_along_axis(plain, (j + r) % M if not inverse else (j - r) % M, axis=1)


def f32_key(v):
    """The lists' distance key (common.h): order-preserving image of the float's bits, every NaN 0xffc00000 (behind +inf)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    u = v.view(np.uint32).astype(np.uint64)
    k = (u ^ np.where(u >> np.uint64(31), np.uint64(0xffffffff), np.uint64(0x80000000))) & np.uint64(0xffffffff)
    return np.where(np.isnan(v), np.uint64(0xffc00000), k)


def bitmap(valid):
    """bool [N] -> the validity bitmap i32 [ceil(N / 32) + 2], bit n % 32 of word n / 32"""
    N = valid.size
    b = np.zeros(((N + 31) // 32 + 2) * 32, bool)
    b[:N] = valid
    return np.packbits(b.reshape(-1, 32), axis=1, bitorder='little').view(np.int32).reshape(-1)


def fp32_chain_bound(terms, d64, D):
    """|kernel distance - float64 distance| of the exact distance kernels (annlite_exact_gather_dist, rerank_topk_kernel, the float
    graph's rows_dist: one chain), derived in tests/test_rerank_topk.py: ``terms`` f64 [..., D] are t_j = (x_j - q_j)^2 (EUCLIDEAN)
    or x_j q_j, ``d64`` their sum (or 1 - sum).  ceil(D / 64) fma terms per lane, then a 6-level butterfly: (2 D + 4) u sum|t_j|
    + u |d| with u = 2^-24 (the 2 D covers the chains and the rounding of x_j - q_j, the last term 1 - s)."""
    u = 2.0 ** -24
    return (2 * D + 4) * u * np.abs(terms).sum(-1) + u * np.abs(d64)


# ---- the float graph walk (annlite_graph_f32_search), restated: tests/test_graph_f32_walk.py, tests/test_graph_f32_restated.py ----
def random_links(rs, n, L, full_frac=0.6):
    """Link lists i32 [n, L + 1] (count, ids): ragged and empty lists, near and far neighbours, ids beyond the table, a neighbour
    listed twice."""
    links = np.zeros((n, L + 1), np.uint32)
    cnt = np.where(rs.rand(n) < full_frac, L, rs.randint(0, L + 1, n)).astype(np.uint32)  # ragged and empty lists
    links[:, 0] = cnt
    nb = rs.randint(0, n, size=(n, L)).astype(np.uint32)
    near = (np.arange(n)[:, None] + rs.randint(1, 50, size=(n, L))) % n
    nb = np.where(rs.rand(n, L) < 0.7, near, nb).astype(np.uint32)
    nb[rs.rand(n, L) < 0.002] = n + 5  # beyond the table: never followed
    if L > 1:
        nb[:, 1] = np.where(rs.rand(n) < 0.05, nb[:, 0], nb[:, 1])  # a neighbour listed twice
    links[:, 1:] = nb
    return links.view(np.int32)


def key_to_bits(k):
    """inverse of the list's key: the float's own bits (the canonical NaN for the NaN key)"""
    k = int(k)
    return k ^ 0x80000000 if k & 0x80000000 else k ^ 0xffffffff


def _walk_result(lst, cap, ef, valid):
    ids = np.full(ef, -1, np.int64)
    bits_ = np.full(ef, np.float32(np.inf).view(np.uint32), np.uint32)
    for i, t in enumerate(lst[:cap]):
        if valid is None or valid[t[1]]:
            ids[i] = t[1]
            bits_[i] = key_to_bits(t[0])
    return ids, bits_


def walk_restated(links, seeds, keys, ef, valid=None, stats=None):
    """One query.  ``links`` u32 [N, L+1] (count, ids), ``keys`` u64 [N]: f32_key of the query's distance to every row.
    Returns (ids i64 [ef], distance bits u32 [ef]); ``stats`` (a dict) receives the expansions and the rows evaluated."""
    n = keys.shape[0]
    E = 1 if ef <= 64 else 2 if ef <= 128 else 4  # registers per lane of the kernel's list
    slots, cap = 64 * E, min(ef, 64 * E)
    lst = []  # sorted [(key, node, expanded)]: the kernel's list of 64 E entries, `cap` of them live
    seen = set()
    n_expand = n_eval = 0

    def offer(nodes):
        if not len(nodes):
            return
        worst = (lst[cap - 1][0], lst[cap - 1][1]) if len(lst) >= cap else (1 << 40, 1 << 40)
        new = [(int(keys[v]), int(v), False) for v in nodes if (int(keys[v]), int(v)) < worst]
        lst.extend(new)
        lst.sort(key=lambda t: (t[0], t[1]))
        del lst[slots:]

    seeds = [int(s) for s in seeds]
    for s0 in range(0, len(seeds), 64):
        rnd = [s for s in seeds[s0:s0 + 64] if s < n]
        n_eval += len(rnd)
        offer(rnd)
    for t in lst:
        seen.add(t[1])
    while True:
        pick = [i for i, t in enumerate(lst[:cap]) if not t[2]][:1]
        if not pick:
            break
        i = pick[0]
        lst[i] = (lst[i][0], lst[i][1], True)
        n_expand += 1
        fresh = []
        row = links[lst[i][1]]
        for nb in row[1:1 + int(row[0])]:
            nb = int(nb)
            if nb < n and nb not in seen:
                seen.add(nb)
                fresh.append(nb)
        n_eval += len(fresh)
        offer(fresh)
    if stats is not None:
        stats.update(expansions=n_expand, evals=n_eval)
    return _walk_result(lst, cap, ef, valid)


def walk_forgetful(links, seeds, keys, ef, table, valid=None, stats=None):
    """The same rule with a visited table that cannot hold the walk (Beam::visit once its buckets are full): it records at most
    ``table`` nodes (None: every node) and reports every other node as new, each time it is met.  What then keeps the list right
    is the merge alone: of the offered (key, node) that beat the list's worst entry, one that stands anywhere in the 64 E-slot
    list already, or that came earlier in the same offer, is dropped.  A node that was evaluated before and is NOT in the list
    did not beat the worst entry then, or was pushed out behind slot 64 E since, and the worst entry only falls: it loses again."""
    n = keys.shape[0]
    E = 1 if ef <= 64 else 2 if ef <= 128 else 4
    slots, cap = 64 * E, min(ef, 64 * E)
    lst = []
    seen = set()
    n_expand = n_eval = 0

    def visit(v):  # True: not seen before, as far as the table knows
        if v in seen:
            return False
        if table is None or len(seen) < table:
            seen.add(v)
        return True

    def offer(nodes):
        if not len(nodes):
            return
        worst = (lst[cap - 1][0], lst[cap - 1][1]) if len(lst) >= cap else (1 << 40, 1 << 40)
        have = {(t[0], t[1]) for t in lst}
        for v in nodes:
            kv = (int(keys[v]), int(v))
            if kv < worst and kv not in have:
                have.add(kv)
                lst.append((kv[0], kv[1], False))
        lst.sort(key=lambda t: (t[0], t[1]))
        del lst[slots:]

    seeds = [int(s) for s in seeds]
    for s0 in range(0, len(seeds), 64):
        rnd = [s for s in seeds[s0:s0 + 64] if s < n]
        n_eval += len(rnd)
        offer(rnd)
    for t in list(lst):
        visit(t[1])
    while True:
        pick = [i for i, t in enumerate(lst[:cap]) if not t[2]][:1]
        if not pick:
            break
        i = pick[0]
        lst[i] = (lst[i][0], lst[i][1], True)
        n_expand += 1
        row = links[lst[i][1]]
        fresh = [int(nb) for nb in row[1:1 + int(row[0])] if int(nb) < n and visit(int(nb))]
        n_eval += len(fresh)
        offer(fresh)
    if stats is not None:
        stats.update(expansions=n_expand, evals=n_eval)
    return _walk_result(lst, cap, ef, valid)
