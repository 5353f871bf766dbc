"""The stages of the pruned search around its scan (ivf.hip), each on arrays the test builds itself -- no scan runs, every
branch is reached on purpose: ``ivf_plan_kernel`` (both entry points), ``ivf_rescore_kernel``, ``ivf_candidate_ids_kernel``,
``ivf_merge_lists_kernel``.

References: the plan is checked against the invariants the scan relies on (``check_plan``, numpy); the re-score against the
oracle's gathered ADC sums + its top-k on (sum, external id); the merge against the oracle's top-k over the lists' pairs.  The
numpy pieces (``check_plan``, ``f32_key``) are themselves run on the CPU first, against a brute-force planner / the NaN-last sort."""
import numpy as np
import pytest

from _refs import NANS, bitmap as _bitmap, bits as _bits, f32_key, lexsort_nan_last, on_gpu, topk_pairs

OVERFLOW = 0xffffffff


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


# ------------------------------------------------------------------------------------------- references (numpy)
def check_plan(cells, C, qt, cell_rows, order, n_first, vmap, slot_of, tile_rows, n_used, T):
    """What the scan relies on; raises AssertionError with the name of the broken invariant."""
    B, P = cells.shape
    n_first = 0 if n_first >= P else n_first
    assert vmap.shape == (T * qt,) and tile_rows.shape == (T, 2) and 0 <= n_used <= T, 'extent'
    s = slot_of.ravel().astype(np.int64)
    assert s.min() >= 0 and s.max() < n_used * qt, 'slot inside the used tiles'
    assert np.unique(s).size == B * P, 'one slot per pair'
    q_of = np.repeat(np.arange(B), P)
    assert np.array_equal(vmap[s], q_of), 'vmap[slot] is the query'
    assert (vmap >= 0).sum() == B * P and (vmap[vmap < 0] == -1).all(), 'every other slot is -1'
    assert np.array_equal(tile_rows[s // qt], cell_rows[cells.ravel()]), "the tile carries its cell's rows"
    assert (tile_rows[n_used:] == -1).all(), 'unused tiles are (-1, -1)'
    # virtual cell of a pair: its cell, in the second class (C + cell) when its probe rank is >= n_first > 0
    p_of = np.tile(np.arange(P), B)
    vc = cells.ravel().astype(np.int64) + (C if n_first > 0 else 0) * (p_of >= n_first)
    tile_vc = np.full(n_used, -1, np.int64)
    tile_vc[s // qt] = vc
    assert (tile_vc >= 0).all(), 'no used tile without a pair'
    assert np.array_equal(tile_vc[s // qt], vc), 'a tile serves one (class, cell)'
    # cells in `order` (the first class, then the second), the tiles of a cell back to back, ceil(pairs / qt) of them
    vorder = np.concatenate([order, C + order]) if n_first > 0 else order.astype(np.int64)
    rank = np.empty(vorder.size, np.int64)
    rank[vorder] = np.arange(vorder.size)
    assert (np.diff(rank[tile_vc]) >= 0).all(), 'tiles follow cell_order, one run per cell'
    cnt = np.bincount(vc, minlength=vorder.size)
    assert np.array_equal(np.bincount(tile_vc, minlength=vorder.size), -(-cnt // qt)), 'ceil(pairs / qt) tiles per cell'


def plan_brute_force(cells, C, qt, cell_rows, order, n_first, T):
    """A planner in plain loops (pairs in index order): one valid plan, to run check_plan on without a GPU."""
    B, P = cells.shape
    n_first = 0 if n_first >= P else n_first
    vmap = np.full(T * qt, -1, np.int32)
    slot_of = np.zeros((B, P), np.int32)
    tile_rows = np.full((T, 2), -1, np.int64)
    t = 0
    for cls in ((0, 1) if n_first > 0 else (0,)):
        for c in order:
            pairs = [(b, p) for b in range(B) for p in range(P)
                     if cells[b, p] == c and (n_first == 0 or (p >= n_first) == bool(cls))]
            for r, (b, p) in enumerate(pairs):
                v = (t + r // qt) * qt + r % qt
                slot_of[b, p], vmap[v] = v, b
                tile_rows[t + r // qt] = cell_rows[c]
            t += -(-len(pairs) // qt)
    return vmap, slot_of, tile_rows, t


def _plan_inputs(rs, B, P, C, pattern):
    if pattern == 'one_cell':
        cells = np.tile(rs.permutation(C)[:P][None, :], (B, 1))
    elif pattern == 'each_once':
        assert B * P == C
        cells = rs.permutation(C).reshape(B, P)
    else:
        hot = min(C, max(P, 1 + C // 8))  # most probes go to a few cells: full tiles and partly filled ones
        cells = np.stack([rs.permutation(C if b % 3 == 0 else hot)[:P] for b in range(B)])
    sizes = rs.randint(0, 500, size=C) * (rs.rand(C) < 0.8)  # a fifth of the cells empty
    begin = np.cumsum((sizes + 63) // 64 * 64) - (sizes + 63) // 64 * 64
    cell_rows = np.stack([begin, begin + sizes], 1).astype(np.int64)
    order = np.argsort(-sizes, kind='stable').astype(np.int32)
    return cells.astype(np.int32), cell_rows, order


def _max_tiles(B, P, C, qt, n_first):
    pairs = B * P
    return pairs // qt + min((2 * C) if 0 < n_first < P else C, pairs)


# ------------------------------------------------------------------------------------------- CPU: the references themselves
@pytest.mark.parametrize('B,P,C,qt,n_first,pattern', [(9, 3, 7, 2, 0, 'mixed'), (9, 3, 7, 2, 1, 'mixed'), (9, 3, 7, 4, 2, 'mixed'),
                                                      (9, 3, 7, 4, 3, 'mixed'), (5, 1, 1, 1, 0, 'one_cell'), (2, 4, 8, 16, 1, 'each_once')])
def test_reference_plan_checker_accepts_a_brute_force_plan_and_rejects_broken_ones(B, P, C, qt, n_first, pattern):
    rs = np.random.RandomState(B + C + qt + n_first)
    cells, cell_rows, order = _plan_inputs(rs, B, P, C, pattern)
    T = _max_tiles(B, P, C, qt, n_first)
    vmap, slot_of, tile_rows, used = plan_brute_force(cells, C, qt, cell_rows, order, n_first, T)
    assert used <= T
    args = (cells, C, qt, cell_rows, order, n_first)
    check_plan(*args, vmap, slot_of, tile_rows, used, T)

    def broken(**kw):
        state = dict(vmap=vmap.copy(), slot_of=slot_of.copy(), tile_rows=tile_rows.copy(), used=used)
        for name, f in kw.items():
            state[name] = f(state[name])
        with pytest.raises(AssertionError):
            check_plan(*args, state['vmap'], state['slot_of'], state['tile_rows'], state['used'], T)

    def two_pairs_one_slot(s):
        s.reshape(-1)[0] = s.reshape(-1)[-1]
        return s

    def wrong_query(v):
        v[slot_of[0, 0]] = B - 1 if B > 1 else -1
        return v

    def stray_slot(v):
        v[np.nonzero(v < 0)[0][0]] = 0
        return v

    def wrong_rows(t):
        t[0, 1] += 1
        return t

    broken(slot_of=two_pairs_one_slot)
    broken(vmap=wrong_query)
    broken(tile_rows=wrong_rows)
    broken(used=lambda u: u + 1)       # a used tile without a pair
    if (vmap < 0).any():
        broken(vmap=stray_slot)
    if np.unique(cells).size > 1:      # the cells walked in another order: a valid plan for THAT order only
        v2, s2, t2, u2 = plan_brute_force(cells, C, qt, cell_rows, order[::-1], n_first, T)
        check_plan(cells, C, qt, cell_rows, order[::-1], n_first, v2, s2, t2, u2, T)
        with pytest.raises(AssertionError):
            check_plan(*args, v2, s2, t2, u2, T)


def test_reference_key_orders_like_the_nan_last_sort():
    rs = np.random.RandomState(1)
    v = np.concatenate([rs.randn(50).astype(np.float32), NANS, _bits(0x7f800000, 0xff800000, 0x00000000, 0x00000001, 0x80000001),
                        np.float32([1, 1, 2, 2])])
    ids = rs.permutation(v.size)
    k = f32_key(v)
    assert np.array_equal(np.lexsort((ids, k)), lexsort_nan_last(v, ids))
    assert k.max() == 0xffc00000 and (k[np.isnan(v)] == 0xffc00000).all() and f32_key(np.float32([np.inf]))[0] < 0xffc00000


# ------------------------------------------------------------------------------------------- GPU: the plan
PLAN_CASES = [  # B, P, C, qt, pattern.  Pairs stay in registers up to 1024 * kReg = 24576; the cells' rows while ceil(Cv / 1024) <= kCellReg = 4
    (1, 1, 1, 1, 'one_cell'),
    (123, 5, 7, 16, 'mixed'),
    (123, 5, 37, 32, 'mixed'),
    (1000, 1, 256, 16, 'one_cell'),       # every query probes the same cell: 63 tiles of one cell
    (64, 4, 256, 1, 'each_once'),         # every cell probed exactly once
    (1536, 16, 256, 32, 'mixed'),         # 24576 pairs: the last count that stays in registers
    (1537, 16, 4096, 16, 'mixed'),        # 24592 pairs: through memory; 4096 cells in registers (8192 virtual ones are not)
    (700, 8, 4097, 16, 'mixed'),          # one cell more: the cells' loop through memory
    (300, 7, 16384, 32, 'mixed'),         # the largest cell count
]


@on_gpu
@pytest.mark.parametrize('B,P,C,qt,pattern', PLAN_CASES)
def test_plan_keeps_the_invariants_of_the_scan(ops, B, P, C, qt, pattern):
    rs = np.random.RandomState(B + P + C + qt)
    cells, cell_rows, order = _plan_inputs(rs, B, P, C, pattern)
    cd, rd, od = ops.to_dev(cells), ops.to_dev(cell_rows), ops.to_dev(order)
    for n_first in sorted({0, 1, P - 1, P}):
        if 0 < n_first < P and C == 16384:  # two classes of 16384 cells: 262 KB of counters, the entry point refuses
            with pytest.raises(AssertionError):
                ops.ivf_plan_first(cd, C, qt, rd, od, n_first)
            continue
        T = ops.ivf_max_tiles_first(B, P, C, qt) if 0 < n_first < P else ops.ivf_max_tiles(B, P, C, qt)
        assert T == _max_tiles(B, P, C, qt, n_first)
        outs = [ops.ivf_plan_first(cd, C, qt, rd, od, n_first)]
        if n_first == 0:
            outs.append(ops.ivf_plan(cd, C, qt, rd, od))
        for vmap, slot_of, tile_rows, used in outs:
            check_plan(cells, C, qt, cell_rows, order, n_first, vmap.cpu().numpy(), slot_of.cpu().numpy(), tile_rows.cpu().numpy(),
                       int(used.item()), T)


@on_gpu
def test_plan_first_refuses_cell_counts_whose_counters_do_not_fit_the_lds(ops):
    """Two classes double the counters: (2 * 2 C + 16) * 4 bytes of LDS.  C = 10236 is the last count that fits 160 KB; above
    it the entry point returns ANNLITE_ERR_INVALID and launches nothing (the outputs keep their contents)."""
    import torch

    from annlite_amd import _capi

    rs = np.random.RandomState(7)
    B, P, qt = 40, 4, 16
    for C, ok in ((10236, True), (10237, False), (16384, False)):
        assert ((2 * 2 * C + 16) * 4 <= 160 * 1024) == ok
        cells, cell_rows, order = _plan_inputs(rs, B, P, C, 'mixed')
        T = ops.ivf_max_tiles_first(B, P, C, qt)
        dev = ops.device()
        vmap = torch.full((T * qt,), -7, dtype=torch.int32, device=dev)
        slot_of = torch.full((B, P), -7, dtype=torch.int32, device=dev)
        tile_rows = torch.full((T, 2), -7, dtype=torch.int64, device=dev)
        used = torch.full((1,), -7, dtype=torch.int32, device=dev)
        cd, rd, od = ops.to_dev(cells), ops.to_dev(cell_rows), ops.to_dev(order)
        rc = _capi.lib().annlite_ivf_plan_first(cd.data_ptr(), B, P, C, qt, rd.data_ptr(), od.data_ptr(), T, vmap.data_ptr(),
                                                slot_of.data_ptr(), tile_rows.data_ptr(), used.data_ptr(), 1, _capi.stream_ptr())
        torch.cuda.synchronize()
        if ok:
            assert rc == 0
            check_plan(cells, C, qt, cell_rows, order, 1, vmap.cpu().numpy(), slot_of.cpu().numpy(), tile_rows.cpu().numpy(),
                       int(used.item()), T)
        else:
            assert rc == _capi.ERR_INVALID
            assert all((t.cpu().numpy() == -7).all() for t in (vmap, slot_of, tile_rows, used))
        # one class of the same cells is served either way
        v, s, t, u = ops.ivf_plan_first(cd, C, qt, rd, od, 0)
        check_plan(cells, C, qt, cell_rows, order, 0, v.cpu().numpy(), s.cpu().numpy(), t.cpu().numpy(), int(u.item()), ops.ivf_max_tiles(B, P, C, qt))


# ------------------------------------------------------------------------------------------- GPU: re-score, candidate ids
def _stage_arrays(rs, B, P, C, M, Ks, qt, cand_cap, long_list=False):
    """A cell-sorted table of C cells, B queries probing P distinct cells each, one slot per (query, probe) inside its own tile of
    qt slots, and per slot a candidate list: rows of its cell (distinct, every index < N), empty, or overflowed."""
    sizes = rs.randint(1, 90, size=C)
    if long_list:
        sizes[0] = 700
    begin = np.cumsum(sizes) - sizes
    N = int(sizes.sum())
    cell_rows = np.stack([begin, begin + sizes], 1).astype(np.int64)
    codes = rs.randint(0, Ks, size=(N, M)).astype(np.uint8)
    codes[begin[C - 1]:begin[C - 1] + min(sizes[C - 1], sizes[0])] = codes[:min(sizes[C - 1], sizes[0])]  # the same code rows in two cells
    cells = np.stack([rs.permutation(C)[:P] for _ in range(B)]).astype(np.int32)
    cells[0, 0], cells[0, 1:] = 0, (np.arange(1, P) if P > 1 else [])
    if P > 1:
        cells[0, P - 1] = C - 1                         # query 0 probes both copies
    V = B * P * qt
    slot_of = ((np.arange(B * P) * qt) + (np.arange(B * P) % qt)).reshape(B, P).astype(np.int32)
    tile_rows = cell_rows[cells.ravel()]
    cand = np.full((V, cand_cap), 0, np.uint32)
    count = np.zeros(V, np.uint32)
    lists = {}
    for b in range(B):
        for p in range(P):
            rb, re = cell_rows[cells[b, p]]
            mode = rs.randint(0, 6) if b > 1 else (5 if b == 1 else 4)
            if mode == 0:
                rows = np.zeros(0, np.int64)            # nothing passed the filter
            elif mode == 5:
                rows = None                             # overflow: the whole cell, under the validity bitmap
            else:
                n = min(re - rb, cand_cap) if mode == 4 else rs.randint(1, min(re - rb, cand_cap) + 1)
                rows = rb + rs.permutation(re - rb)[:n]
            v = slot_of[b, p]
            if rows is None:
                count[v] = OVERFLOW
                cand[v] = rs.randint(0, N, size=cand_cap)   # not looked at (and in range all the same)
            else:
                count[v] = rows.size
                cand[v, :rows.size] = rows
            lists[b, p] = rows
    return dict(N=N, cells=cells, cell_rows=cell_rows, codes=codes, slot_of=slot_of, tile_rows=tile_rows, cand=cand, count=count,
                lists=lists)


def _tables(rs, kind, B, M, Ks):
    lut = rs.randn(B, M, Ks).astype(np.float32)
    if kind == 'ties':
        lut = rs.randint(0, 3, size=(B, M, Ks)).astype(np.float32)
    elif kind == 'all_inf':
        lut[:, 0, :] = np.inf
    elif kind == 'all_nan':  # every sum NaN, of every sign and payload
        lut[:, M - 1, :] = NANS[rs.randint(0, NANS.size, size=(B, Ks))]
        lut[:, 0, :] = np.where(rs.rand(B, Ks) < 0.5, np.inf, lut[:, 0, :])
    elif kind == 'neg_inf':  # -inf sums for some rows, NaN (inf - inf) for some, numbers for the rest
        lut[:, 1, : max(1, Ks // 8)] = -np.inf
        lut[:, 2, Ks - max(1, Ks // 8):] = np.inf
    return lut


def _rescore_expected(oracle, a, lut, b, k, row_ids, valid, id_base, sqrt):
    P = a['cells'].shape[1]
    rows = []
    for p in range(P):
        r = a['lists'][b, p]
        if r is None:
            rb, re = a['cell_rows'][a['cells'][b, p]]
            r = np.arange(rb, re)
            if valid is not None:
                r = r[valid[r]]
        rows.append(np.asarray(r, np.int64))
    rows = np.concatenate(rows)
    with np.errstate(invalid='ignore'):
        sums = oracle.adc_gather_c(lut[b], a['codes'], rows) if rows.size else np.zeros(0, np.float32)
        ext = row_ids[rows] if row_ids is not None else rows
        assert np.unique(ext).size == ext.size
        d, i = topk_pairs(oracle, sums, ext, k)
        if sqrt:
            d = np.where(i >= 0, np.sqrt(d), d)
    return d, np.where(i >= 0, i + id_base, -1)


RESCORE_CASES = [  # M, Ks, k, P, qt, table kind
    (4, 4, 1, 1, 1, 'ties'), (8, 100, 10, 5, 8, 'random'), (16, 256, 20, 16, 16, 'random'), (32, 256, 64, 5, 4, 'random'),
    (64, 256, 10, 5, 8, 'random'), (16, 100, 64, 16, 1, 'ties'), (8, 4, 20, 5, 8, 'ties'), (16, 256, 10, 5, 16, 'all_inf'),
    (16, 256, 20, 5, 16, 'all_nan'), (32, 100, 10, 16, 8, 'all_nan'), (16, 256, 20, 5, 16, 'neg_inf'), (64, 4, 1, 16, 8, 'neg_inf'),
]


@on_gpu
@pytest.mark.parametrize('M,Ks,k,P,qt,kind', RESCORE_CASES)
def test_rescore_equals_the_oracle_on_the_union_of_the_lists(ops, oracle, M, Ks, k, P, qt, kind):
    rs = np.random.RandomState(M + Ks + k + P)
    B, C = 7, 24
    for cand_cap, long_list in ((256, False), (640, True)):  # a list longer than 256: several rounds per wave
        a = _stage_arrays(rs, B, P, C, M, Ks, qt, cand_cap, long_list)
        N = a['N']
        lut = _tables(rs, kind, B, M, Ks)
        valid = rs.rand(N) < 0.7
        row_ids = (rs.permutation(N) * 3 + 1).astype(np.int64)    # external ids, not the table's order
        dev = {n: ops.to_dev(a[n]) for n in ('codes', 'cand', 'count', 'slot_of', 'tile_rows')}
        for use_ids, use_valid, id_base, sqrt in ((False, False, 0, False), (True, True, (1 << 33) + 7, False), (True, False, 5, True),
                                                  (False, True, 0, True)):
            d, i = ops.ivf_rescore(ops.to_dev(lut), dev['codes'], dev['cand'], dev['count'], dev['slot_of'], dev['tile_rows'], qt, k,
                                   row_ids=ops.to_dev(row_ids) if use_ids else None,
                                   valid_bits=ops.to_dev(_bitmap(valid)) if use_valid else None, id_base=id_base, sqrt=sqrt)
            d, i = d.cpu().numpy(), i.cpu().numpy()
            for b in range(B):
                wd, wi = _rescore_expected(oracle, a, lut, b, k, row_ids if use_ids else None, valid if use_valid else None, id_base, sqrt)
                assert np.array_equal(i[b], wi), (kind, cand_cap, b, use_ids, use_valid, sqrt, i[b][:6], wi[:6])
                assert np.array_equal(d[b], wd, equal_nan=True), (kind, cand_cap, b, use_ids, use_valid, sqrt)


@on_gpu
def test_rescore_of_empty_lists_is_inf_and_minus_one(ops):
    rs = np.random.RandomState(3)
    a = _stage_arrays(rs, 5, 3, 8, 16, 256, 4, 256)
    a['count'][:] = 0
    lut = rs.randn(5, 16, 256).astype(np.float32)
    d, i = ops.ivf_rescore(ops.to_dev(lut), ops.to_dev(a['codes']), ops.to_dev(a['cand']), ops.to_dev(a['count']),
                           ops.to_dev(a['slot_of']), ops.to_dev(a['tile_rows']), 4, 10, id_base=9, sqrt=True)
    assert (i.cpu().numpy() == -1).all() and np.isposinf(d.cpu().numpy()).all()


@on_gpu
@pytest.mark.parametrize('B', [1, 6, 9])
def test_candidate_ids_concatenates_the_lists_in_probe_order(ops, B):
    rs = np.random.RandomState(B)
    P, C, qt, cap = 4, 12, 4, 256
    a = _stage_arrays(rs, B, P, C, 4, 4, qt, cap)
    N = a['N']
    row_ids = (rs.permutation(N) * 3 + 1).astype(np.int64)
    dev = {n: ops.to_dev(a[n]) for n in ('cand', 'count', 'slot_of')}
    lens = np.array([[0 if a['lists'][b, p] is None else a['lists'][b, p].size for p in range(P)] for b in range(B)])
    first, total = int(lens[0, 0]), int(lens[0].sum())
    for R in sorted({1, max(1, first - 1), first + 1, max(1, total), total + 5, 700}):  # below the first list, the total, beyond
        for use_ids, id_base in ((False, 0), (True, (1 << 33) + 1)):
            got = ops.ivf_candidate_ids(dev['cand'], dev['count'], dev['slot_of'], R, row_ids=ops.to_dev(row_ids) if use_ids else None,
                                        id_base=id_base).cpu().numpy()
            for b in range(B):
                rows = np.concatenate([np.zeros(0, np.int64)] + [a['cand'][a['slot_of'][b, p], :lens[b, p]].astype(np.int64) for p in range(P)])
                ext = (row_ids[rows] if use_ids else rows) + id_base
                want = np.full(R, -1, np.int64)
                want[:min(R, ext.size)] = ext[:R]
                assert np.array_equal(got[b], want), (B, R, b, use_ids)


# ------------------------------------------------------------------------------------------- GPU: merge of the per-cell lists
@on_gpu
@pytest.mark.parametrize('P,k', [(1, 1), (5, 1), (3, 10), (7, 10), (16, 16), (5, 64), (3, 50), (1, 64)])
def test_merge_lists_equals_the_oracle_over_the_pairs(ops, oracle, P, k):
    rs = np.random.RandomState(10 * P + k)
    B, C, qt = 9, 20, 4
    a = _stage_arrays(rs, B, P, C, 4, 4, qt, 256)
    N, V = a['N'], B * P * qt
    # external ids ascending inside a cell (the merge's contract), the cells' id ranges in reverse table order
    row_ids = np.empty(N, np.int64)
    top = 4 * N
    for c in range(C):
        rb, re = a['cell_rows'][c]
        top -= 3 * (re - rb) + 1
        row_ids[rb:re] = top + np.sort(rs.permutation(3 * (re - rb))[:re - rb])
    pool = np.concatenate([np.float32([0.0, 0.5, 0.5, 1.0, 4.0, np.inf, -1.0, -np.inf]), NANS[:3]])
    lists = np.full((V, k), -1, np.int64)  # all-ones keys: no entry
    pairs = {}
    for b in range(B):
        for p in range(P):
            rb, re = a['cell_rows'][a['cells'][b, p]]
            n = [0, 1, min(k, re - rb)][rs.randint(0, 3)] if b % 3 else (0 if b == 3 else min(k, re - rb))
            rows = rb + np.sort(rs.permutation(re - rb)[:n])
            vals = pool[rs.randint(0, pool.size, size=n)] if b != 6 else np.full(n, 0.5, np.float32)  # query 6: every key equal
            o = np.lexsort((rows, f32_key(vals)))       # a slot's list: ascending in (key, table row)
            rows, vals = rows[o], vals[o]
            lists[a['slot_of'][b, p], :n] = ((f32_key(vals) << np.uint64(32)) | rows.astype(np.uint64)).view(np.int64)
            pairs[b, p] = (vals, rows)
    ld, sd = ops.to_dev(lists), ops.to_dev(a['slot_of'])
    for use_ids, id_base, sqrt in ((True, (1 << 33) + 3, False), (False, 0, False), (True, 0, True)):
        d, i = ops.ivf_merge_lists(ld, sd, k, row_ids=ops.to_dev(row_ids) if use_ids else None, id_base=id_base, sqrt=sqrt)
        d, i = d.cpu().numpy(), i.cpu().numpy()
        for b in range(B):
            vals = np.concatenate([pairs[b, p][0] for p in range(P)])
            rows = np.concatenate([pairs[b, p][1] for p in range(P)])
            wd, wi = topk_pairs(oracle, vals, row_ids[rows] if use_ids else rows, k)
            with np.errstate(invalid='ignore'):
                wd = np.where(wi >= 0, np.sqrt(wd), wd) if sqrt else wd
            wi = np.where(wi >= 0, wi + id_base, -1)
            assert np.array_equal(i[b], wi), (P, k, b, use_ids, sqrt, i[b][:6], wi[:6])
            assert np.array_equal(d[b], wd, equal_nan=True), (P, k, b, use_ids, sqrt)
    assert (i[3] == -1).all()  # the query whose every list is empty
