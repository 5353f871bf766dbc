"""Pages of the document listing on the device (page.hip).

Kernel level: ``ops.order_page`` / ``ops.bitmap_page`` over tensors built here, against numpy -- ``np.lexsort`` over (class, key, row) of
the selected rows, the keys made with ``columns.order_key`` -- for equality: the order is exact by construction.

Facade level: two facades over the same rows, one with ``filter_eval='auto'`` and one reopened with ``filter_eval='host'`` (whose
``filter()`` is the specification); every page of the grid is the same documents in the same order."""
import struct

import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

I64, F64, CODE = 0, 1, 2
BIG = 100003
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
SUB = struct.unpack('<d', struct.pack('<Q', 1))[0]
FMAX = float(np.finfo(np.float64).max)


# ------------------------------------------------------------------------------------------------ kernel level
def _block_rows():
    from annlite_amd import _capi

    return _capi.PAGE_BLOCK_ROWS


def _words(flags, n_words, fill_behind=True):
    """bool [N] -> i32 [n_words] on the device; the bits behind N are SET where ``fill_behind``: nothing may read them"""
    import torch

    bits = np.full((n_words * 32,), fill_behind, dtype=bool)
    bits[: flags.size] = flags
    return torch.from_numpy(np.packbits(bits, bitorder='little').view('<u4').view(np.int32).copy()).cuda()


class Table:
    """one column over N rows in arrays of a larger capacity, with garbage behind the rows"""

    def __init__(self, kind, values, present=None, rows=None, words=None, extra=77):
        import torch

        from annlite_amd.columns import order_key, rank_table

        self.kind, self.N = kind, len(values)
        N, cap = self.N, len(values) + extra
        self.n_words = (cap + 31) // 32 + 2
        self.present = np.ones((N,), dtype=bool) if present is None else np.asarray(present, dtype=bool)
        self.rows = np.ones((N,), dtype=bool) if rows is None else np.asarray(rows, dtype=bool)
        rs = np.random.RandomState(3)
        if kind == CODE:
            self.rank_host = rank_table(words)
            keys = [int(self.rank_host[c]) for c in values]
            dev = np.concatenate([np.asarray(values, dtype=np.int32), rs.randint(0, 2 ** 31 - 1, size=extra).astype(np.int32)])
            self.rank = torch.from_numpy(self.rank_host).cuda()
        else:
            dtype = np.int64 if kind == I64 else np.float64
            cache = {}
            keys = []
            for v in values:  # (order_key per distinct value: Python's hash has -0.0 == 0.0 == 0 share an entry, as they share a key)
                k = cache.get(v)
                if k is None:
                    k = cache[v] = order_key(kind, v)
                keys.append(k)
            garbage = rs.randint(INT64_MIN, INT64_MAX, size=extra, dtype=np.int64).view(dtype)
            dev = np.concatenate([np.asarray(values, dtype=dtype), garbage])
            self.rank = None
        self.keys = np.asarray(keys, dtype=np.uint64)
        self.values_dev = torch.from_numpy(dev).cuda()
        self.present_dev = _words(self.present, self.n_words)
        self.rows_dev = _words(self.rows, self.n_words)

    def mask_dev(self, mask):
        return None if mask is None else _words(np.asarray(mask, dtype=bool), self.n_words)

    def listing(self, mask, descending):
        """the whole listing, by numpy"""
        sel = self.rows if mask is None else self.rows & np.asarray(mask, dtype=bool)
        rows = np.nonzero(sel)[0]
        has = self.present[rows]
        keys = self.keys[rows]
        keys = np.where(has, ~keys if descending else keys, np.uint64(0))
        cls = has ^ bool(descending)  # NULLs: class 0 ascending, class 1 descending
        return rows[np.lexsort((rows, keys, cls))]

    def check(self, mask, pages, directions=(False, True), max_blocks=0, workspace=None):
        from annlite_amd import ops

        mask_dev = self.mask_dev(mask)
        for descending in directions:
            want_all = self.listing(mask, descending)
            assert want_all.size == 0 or want_all.max() < self.N
            for first, count in pages(want_all.size) if callable(pages) else pages:
                rows, n = ops.order_page(mask_dev, self.rows_dev, self.values_dev, self.kind, self.present_dev, self.N, self.n_words, descending,
                                         first, count, rank=self.rank, max_blocks=max_blocks, workspace=workspace)
                assert str(rows.dtype) == 'torch.int32' and rows.numel() == count and n.numel() == 1
                n = int(n.item())
                want = want_all[first: first + count]
                assert n == want.size, (self.N, descending, first, count, n, want.size)
                got = rows[:n].cpu().numpy()
                assert np.array_equal(got, want), (self.N, descending, first, count, got[:8], want[:8])


def _pages(total):
    """the bounds of a page: the first rows, a page inside, the last rows, a short page, first at and beyond the total, one row, the
    largest page"""
    firsts = sorted({0, 1, total // 2, max(total - 1, 0), total, total + 5})
    return [(f, c) for f in firsts for c in (1, 7, 4096)]


def _mixed(N, seed=0):
    """(values with many ties, present: every third row NULL, rows: a few cleared, mask: about half)"""
    rs = np.random.RandomState(100 + N + seed)
    values = rs.randint(-5, 6, size=N).astype(np.int64) * (1 << 40) + rs.randint(0, 3, size=N)
    present = np.arange(N) % 3 != 1
    rows = rs.rand(N) > 0.1
    mask = rs.rand(N) > 0.5
    return values.tolist(), present, rows, mask


@pytest.mark.parametrize('N', [1, 31, 32, 33, 63, 64, 65])
def test_order_page_word_and_wave_edges(N):
    values, present, rows, mask = _mixed(N)
    for kind, vals in ((I64, values), (F64, [v / 8 for v in values])):
        t = Table(kind, vals, present, rows)
        t.check(mask, _pages)
        t.check(None, _pages)
        Table(kind, vals).check(None, _pages)  # every row, no NULL


@pytest.mark.parametrize('delta', [-1, 0, 1])
def test_order_page_workgroup_edge(delta):
    N = _block_rows() + delta
    values, present, rows, mask = _mixed(N)
    t = Table(I64, values, present, rows)
    t.check(mask, _pages)
    t.check(None, _pages, max_blocks=1)
    # NULLs: every third row; pages wholly in the NULL block, across its boundary and wholly outside it, in both directions
    t = Table(F64, [v / 8 for v in values], present)
    nulls, have = int((~present).sum()), int(present.sum())
    t.check(None, [(0, 100), (nulls - 100, 100), (nulls - 3, 10), (nulls, 10), (nulls + 50, 4096)], directions=(False,))
    t.check(None, [(0, 100), (have - 100, 100), (have - 3, 10), (have, 10), (have + 50, 4096)], directions=(True,))
    # ... no NULL, and nothing but NULLs (the rows decide alone)
    Table(I64, values).check(mask, _pages)
    Table(I64, values, np.zeros((N,), dtype=bool)).check(mask, _pages)


@pytest.fixture(scope='module')
def big():
    """tables of 100003 rows, made once"""
    rs = np.random.RandomState(11)
    N = BIG
    present = np.arange(N) % 3 != 2
    three = rs.randint(0, 3, size=N)
    return {
        'equal': Table(I64, [42] * N),
        'low': Table(I64, rs.randint(0, 256, size=N).tolist(), present),
        'high': Table(I64, ((rs.randint(0, 256, size=N).astype(np.int64) - 128) << 56).tolist(), present),
        'three': Table(F64, np.asarray([-1.5, 0.0, 1e300])[three].tolist()),
        'three_counts': np.bincount(three, minlength=3),
        'sorted': Table(I64, list(range(-50000, N - 50000))),
        'reverse': Table(F64, [float(N - i) / 4 for i in range(N)], present),
        'mask': rs.rand(N) > 0.5,
    }


def test_order_page_equal_keys_the_rows_decide(big):
    t = big['equal']
    # 65530 + 12 crosses a 16-bit boundary of the row, 255 + 2 an 8-bit one
    t.check(None, [(65530, 12), (255, 2), (0, 4096), (BIG - 5, 10), (BIG, 3), (BIG + 1, 1), (65535, 1), (65536, 1)])
    t.check(big['mask'], [(65530, 12), (255, 2), (0, 1)])


def test_order_page_one_byte_of_the_key(big):
    for name in ('low', 'high'):
        big[name].check(None, [(0, 10), (33333, 12), (50000, 4096), (BIG - 7, 10)])
        big[name].check(big['mask'], [(0, 10), (25000, 100)])


def test_order_page_three_values_pages_across_a_tie_group(big):
    t, (c0, c1, c2) = big['three'], big['three_counts']
    assert c0 > 4096 and c1 > 4096 and c2 > 4096
    t.check(None, [(c0 - 3, 10), (c0, 10), (c0 + c1 - 4000, 4096), (c0 + c1 - 1, 2), (0, 4096), (c0 // 2, 4096)], directions=(False,))
    t.check(None, [(c2 - 3, 10), (c2, 10), (c2 + c1 - 4000, 4096), (c2 + c1 - 1, 2), (BIG - 4000, 4096)], directions=(True,))


def test_order_page_sorted_and_reverse_sorted(big):
    for name in ('sorted', 'reverse'):
        big[name].check(None, [(0, 10), (70000, 300), (BIG - 100, 4096)])
        big[name].check(big['mask'], [(0, 10), (40000, 300)])


def test_order_page_many_strides_of_one_workgroup(big):
    """``max_blocks=1``: one workgroup strides over all 100003 rows"""
    big['low'].check(big['mask'], [(0, 10), (20000, 4096), (49000, 4096)], max_blocks=1)
    big['three'].check(None, [(int(big['three_counts'][0]) - 3, 10)], max_blocks=1)
    big['equal'].check(None, [(65530, 12)], max_blocks=3)


def test_order_page_4096_rows_of_100003_and_fewer(big):
    t = big['low']
    t.check(None, [(0, 4096), (BIG - 4096, 4096), (BIG - 4095, 4096), (BIG - 17, 4096)])
    few = np.zeros((BIG,), dtype=bool)
    few[::41] = True  # 2440 rows: a page of 4096 that holds fewer
    t.check(few, [(0, 4096), (2000, 4096)])


def test_order_page_edge_values():
    i_edge = [INT64_MIN, -1, 0, 1, INT64_MAX]
    f_edge = [float('-inf'), -FMAX, -SUB, -0.0, 0.0, SUB, float(2 ** 53), FMAX, float('inf')]
    rs = np.random.RandomState(5)
    for kind, edge in ((I64, i_edge), (F64, f_edge)):
        values = [edge[i] for i in rs.randint(0, len(edge), size=300)]
        present = rs.rand(300) > 0.2
        Table(kind, values, present).check(None, _pages)
        Table(kind, edge).check(None, [(0, 4096), (2, 3)])
    # -0.0 and 0.0 tie: the row decides, in both directions
    t = Table(F64, [0.0, -0.0, 0.0, -0.0, -SUB, SUB])
    assert t.listing(None, False).tolist() == [4, 0, 1, 2, 3, 5] and t.listing(None, True).tolist() == [5, 0, 1, 2, 3, 4]
    t.check(None, [(0, 6), (1, 4)])


def test_order_page_dictionary_columns():
    rs = np.random.RandomState(6)
    words = ['b', 'a', 'é', '', 'B', 'aa', 'never']  # (insertion order is not the sorted order; no row has code 6)
    for N in (65, 2000):
        codes = rs.randint(0, 6, size=N).tolist()
        present = rs.rand(N) > 0.25
        Table(CODE, codes, present, words=words).check(rs.rand(N) > 0.3, _pages)
    Table(CODE, [0] * 500, rs.rand(500) > 0.5, words=['only']).check(None, _pages)
    # more than 256 words: two key digits
    many = ['w%05d' % i for i in rs.permutation(3000)]
    Table(CODE, rs.randint(0, 3000, size=5000).tolist(), rs.rand(5000) > 0.1, words=many).check(rs.rand(5000) > 0.5, _pages)


def test_order_page_masks():
    N = 2000
    values, present, rows, _ = _mixed(N)
    t = Table(I64, values, present, rows)
    last = np.zeros((N,), dtype=bool)
    last[N - 1] = True
    t.rows[N - 1] = True
    t.rows_dev = _words(t.rows, t.n_words)
    every_other = np.arange(N) % 2 == 0
    for mask in (np.zeros((N,), dtype=bool), np.ones((N,), dtype=bool), last, every_other, None):
        t.check(mask, _pages)
    # a row whose row-present bit is cleared never appears, whatever the mask says
    cleared = np.nonzero(~t.rows)[0]
    assert cleared.size > 50
    for mask in (np.ones((N,), dtype=bool), None):
        for descending in (False, True):
            assert not set(t.listing(mask, descending).tolist()) & set(cleared.tolist())


def test_order_page_is_deterministic_and_shares_a_workspace(big):
    from annlite_amd import ops

    t, ws = big['three'], ops.ScanWorkspace()
    c0 = int(big['three_counts'][0])
    seen = []
    for _ in range(3):
        rows, n = ops.order_page(None, t.rows_dev, t.values_dev, t.kind, t.present_dev, t.N, t.n_words, False, c0 - 2000, 4096, workspace=ws)
        seen.append((rows.cpu().numpy().copy(), int(n.item())))
    assert all(s[1] == 4096 and np.array_equal(s[0], seen[0][0]) for s in seen)
    t.check(big['mask'], [(100, 50)], workspace=ws)


def test_page_errors_launch_nothing():
    import torch

    from annlite_amd import ops

    t = Table(I64, list(range(100)))
    canary = torch.full((4098,), -7, dtype=torch.int32, device='cuda')

    def order(first, count, kind=I64, n_words=None):
        return ops.order_page(None, t.rows_dev, t.values_dev, kind, t.present_dev, t.N, t.n_words if n_words is None else n_words, False, first,
                              count, out=canary[: count + 1])

    for first, count, kw, match in ((0, 4097, {}, 'bad count'), (0, 0, {}, 'bad count'), (-1, 10, {}, 'bad first'), (0, 10, dict(kind=3), 'bad column kind'),
                                    (0, 10, dict(n_words=3), 'bad N'), (2 ** 31 - 5, 10, {}, r'first \+ count')):
        with pytest.raises(AssertionError, match='order_page: ' + match):
            order(first, count, **kw)
    for first, count, match in ((0, 4097, 'bad count'), (0, 0, 'bad count'), (-1, 10, 'bad first')):
        with pytest.raises(AssertionError, match='bitmap_page: ' + match):
            ops.bitmap_page(t.rows_dev, t.N, t.n_words, first, count, out=canary[: count + 1])
    with pytest.raises(AssertionError, match='rank table'):
        ops.order_page(None, t.rows_dev, t.values_dev.view(torch.int32), CODE, t.present_dev, t.N, t.n_words, False, 0, 10, out=canary[:11])
    torch.cuda.synchronize()
    assert bool((canary == -7).all())


@pytest.mark.parametrize('N', [1, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, BIG])
def test_bitmap_page(N):
    from annlite_amd import ops

    assert _block_rows() == 1024
    rs = np.random.RandomState(N)
    n_words = (N + 90 + 31) // 32 + 2
    last = np.zeros((N,), dtype=bool)
    last[N - 1] = True
    masks = [rs.rand(N) > 0.5, np.zeros((N,), dtype=bool), np.ones((N,), dtype=bool), last, np.arange(N) % 2 == 0]
    rows = rs.rand(N) > 0.1
    rows_dev = _words(rows, n_words)
    for mask in masks:
        bits = _words(mask, n_words)
        for and_bits, want_all in ((None, np.nonzero(mask)[0]), (rows_dev, np.nonzero(mask & rows)[0])):
            pages = _pages(want_all.size) + ([(65530, 12), (255, 2)] if N == BIG else [])
            for first, count in pages:
                for max_blocks in ((0, 1) if N == BIG and count == 7 else (0,)):
                    got, n = ops.bitmap_page(bits, N, n_words, first, count, and_bits=and_bits, max_blocks=max_blocks)
                    want = want_all[first: first + count]
                    assert int(n.item()) == want.size and np.array_equal(got[: want.size].cpu().numpy(), want), (N, first, count)


# ------------------------------------------------------------------------------------------------ facade level
N, D = 6000, 32
THREE = {'n': 77777}  # selects 3 rows
NOTHING = {'n': {'$gt': 10 ** 6}}
CATS = ['red', 'green', 'blue', 'grey', 'black', 'white', 'rose', 'Rose', '', 'émeraude']


def _world():
    rs = np.random.RandomState(78)
    x = rs.randn(N, D).astype(np.float32)
    q = rs.randn(4, D).astype(np.float32)
    tags = []
    for r in range(N):
        if r % 29 == 4:
            tags.append({})  # a row without tags at all
            continue
        t = {'extra': r % 3}  # (not declared)
        if r % 13 != 5:  # a float column that mixes ints and floats, with -0.0, 0.0 and 0
            t['price'] = [-0.0, 0.0, 0][r % 3] if r % 7 == 0 else float(rs.randint(-200, 200)) / 4 if r % 9 else int(rs.randint(-50, 50))
        if r % 17 != 3:  # an int column with bools
            t['n'] = bool(r & 1) if r % 10 == 0 else int(rs.randint(0, 100))
        if r % 11 != 7:
            t['cat'] = CATS[int(rs.randint(len(CATS)))]
        tags.append(t)
    for r in (100, 2500, 5999):
        tags[r]['n'] = 77777
    return x, q, tags


@pytest.fixture(scope='module')
def world():
    import torch

    torch.cuda.set_device(0)
    return _world()


@pytest.fixture(scope='module')
def pair(world, tmp_path_factory):
    from test_filter_facade_gpu import _pair

    dev, host = _pair(world, tmp_path_factory.mktemp('pages'))
    assert dev.last_filter_page is None and host.last_filter_page is None
    return dev, host


def _ids(docs):
    return [d.id for d in docs]


def _same_pages(dev, host, filters, orders, on='gpu', limits=None):
    for flt in filters:
        total = len(host.filter(flt, limit=0))
        grid = limits or [(1, 0), (10, 0), (25, 7), (4096, 0), (10, max(total - 3, 0)), (10, total), (10, total + 5)]
        for order_by in orders:
            for ascending in (True, False):
                for limit, offset in grid:
                    kw = dict(limit=limit, offset=offset, order_by=order_by, ascending=ascending)
                    got, want = _ids(dev.filter(flt, **kw)), _ids(host.filter(flt, **kw))
                    assert got == want, (flt, kw, got[:5], want[:5])
                    assert dev.last_filter_page == on and host.last_filter_page == 'host', (flt, kw)
                    bare = dev.filter(flt, include_metadata=False, **kw)
                    assert _ids(bare) == want and dev.last_filter_page == on and all(not d.tags for d in bare)
                    assert _ids(dev.get_docs(flt, **kw)) == want and dev.last_filter_page == on
                kw = dict(limit=25, offset=7, order_by=order_by, ascending=ascending)
                assert _ids(host.get_docs(flt, **kw)) == _ids(host.filter(flt, **kw)) and host.last_filter_page == 'host'


def _filters():
    from test_filter_facade_gpu import FILTERS

    return FILTERS + [None, {}, NOTHING, THREE]


@pytest.mark.parametrize('order_by', [None, 'price', 'n', 'cat'])
def test_facade_pages_are_the_host_pages(pair, world, order_by):
    dev, host = pair
    assert len(host.filter(THREE, limit=0)) == 3 and len(host.filter(_filters()[-2], limit=0)) == 0
    _same_pages(dev, host, _filters(), [order_by])


def test_facade_calls_the_host_keeps(pair):
    from test_filter_facade_gpu import FILTERS

    dev, host = pair
    for flt, kw in ((FILTERS[0], dict(limit=0, order_by='n')), (FILTERS[0], dict(limit=4097, order_by='n')), (None, dict(limit=4097)),
                    (FILTERS[1], dict(limit=10, order_by='extra')), (None, dict(limit=10, order_by='extra', ascending=False)),
                    ({'extra': 1, 'n': {'$lt': 50}}, dict(limit=10, order_by='n')), (FILTERS[0], dict(limit=10, offset=-2, order_by='price')),
                    ({}, dict(limit=10, offset=-2))):
        assert _ids(dev.filter(flt, **kw)) == _ids(host.filter(flt, **kw)), (flt, kw)
        assert dev.last_filter_page == 'host' and host.last_filter_page == 'host', (flt, kw)
    assert _ids(dev.filter(FILTERS[0], limit=10, order_by='n')) == _ids(host.filter(FILTERS[0], limit=10, order_by='n'))
    assert dev.last_filter_page == 'gpu'


def test_facade_pages_after_mutations(world, tmp_path):
    from test_filter_facade_gpu import FILTERS, _docs, _pair

    x, q, tags = world
    dev, host = _pair(world, tmp_path)
    orders, filters = [None, 'price', 'n', 'cat'], [FILTERS[0], None]
    grid = [(10, 0), (25, 7), (4096, 0), (10, 2990)]
    gone = [str(v) for v in range(0, 400, 3)] + ['100', '5999']
    upd = [7, 65, 4000]  # (not among the deleted: fresh offsets behind the others)
    new_tags = [{'n': 1, 'price': -0.0, 'cat': 'rose'}, {'cat': 'A'}, {'n': True, 'price': 3}]
    for ann in (dev, host):
        ann.delete(gone)
        ann.update(_docs(x[upd] + 0.5, new_tags, ids=upd))
    _same_pages(dev, host, filters, orders, limits=grid)
    # an index() that grows the column store past its capacity
    cap = dev._columns.capacity
    more = cap - len(dev._columns) + 500
    rs = np.random.RandomState(4)
    extra = [{'n': int(rs.randint(0, 100)), 'price': float(rs.randint(0, 50)), 'cat': 'new%d' % (i % 5)} if i % 4 else {} for i in range(more)]
    for ann in (dev, host):
        ann.index(_docs(rs.randn(more, D).astype(np.float32), extra, ids=range(10 ** 6, 10 ** 6 + more)))
    assert dev._columns.capacity > cap
    _same_pages(dev, host, filters, orders, limits=grid + [(10, cap - 200), (50, len(dev._columns) - 600)])
    # a batch whose float tag is NaN: the column is irregular, order_by on it goes to the host; the others stay
    for ann in (dev, host):
        ann.index(_docs(x[:2], [{'price': float('nan'), 'n': 5, 'cat': 'red'}, {'price': 1.0, 'n': 6}], ids=['nan0', 'nan1']))
    assert dev._columns.irregular == {'price'}
    _same_pages(dev, host, [FILTERS[0], None], ['price'], on='host', limits=grid)
    _same_pages(dev, host, [FILTERS[0], None], [None, 'n', 'cat'], limits=grid)
