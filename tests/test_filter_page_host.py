"""Pages of the document listing, the host side (columns.py): the 64-bit key the page kernels order by
against Python's own ``sorted``, the rank table of a str column's dictionary, the calls ``ColumnStore.page`` leaves to the host, and
``AnnLite.last_filter_page``.  No GPU."""
import random
import struct

import numpy as np
import pytest

from annlite_amd.columns import CODE, F64, I64, PAGE_MAX, ColumnStore, order_key, rank_table

U64 = 2 ** 64 - 1
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
SUB = struct.unpack('<d', struct.pack('<Q', 1))[0]  # the smallest subnormal
FMAX = float(np.finfo(np.float64).max)


def _values(kind):
    rnd = random.Random(5 + kind)
    if kind == I64:
        edge = [INT64_MIN, INT64_MIN + 1, -1, 0, 1, INT64_MAX - 1, INT64_MAX, True, False]
        return edge + [rnd.randint(INT64_MIN, INT64_MAX) for _ in range(1500)] + [rnd.randint(-40, 40) for _ in range(1500)]
    edge = [float('-inf'), -FMAX, -SUB, -0.0, 0.0, 0, SUB, float(2 ** 53), 2 ** 53, -2 ** 53, FMAX, float('inf'), 1, 1.0, True]
    wide = [struct.unpack('<d', struct.pack('<Q', rnd.getrandbits(64)))[0] for _ in range(1500)]
    return edge + [v for v in wide if v == v] + [rnd.randint(-40, 40) / 4 for _ in range(1000)] + [rnd.randint(-40, 40) for _ in range(500)]


@pytest.mark.parametrize('kind', [I64, F64])
def test_order_key_sorts_as_python_sorts(kind):
    values = _values(kind)
    rnd = random.Random(9)
    rnd.shuffle(values)
    keys = [order_key(kind, v) for v in values]
    assert all(0 <= k <= U64 for k in keys)
    pos = range(len(values))
    up = sorted(pos, key=lambda i: (keys[i], i))
    assert up == sorted(pos, key=values.__getitem__)  # (Python's sort is stable: ties in position)
    assert [values[i] for i in up] == sorted(values)
    down = sorted(pos, key=lambda i: (~keys[i] & U64, i))
    assert down == sorted(pos, key=values.__getitem__, reverse=True)  # (stable under reverse too)
    # equal values, equal keys -- and only those
    for a in values[:60]:
        for b in values[:60]:
            assert (order_key(kind, a) == order_key(kind, b)) == (a == b) and (order_key(kind, a) < order_key(kind, b)) == (a < b)


def test_order_key_ties():
    assert order_key(F64, -0.0) == order_key(F64, 0.0) == order_key(F64, 0) == 1 << 63
    assert order_key(I64, True) == order_key(I64, 1) and order_key(I64, False) == order_key(I64, 0) == 1 << 63
    assert order_key(I64, INT64_MIN) == 0 and order_key(I64, INT64_MAX) == U64
    assert order_key(F64, float('-inf')) < order_key(F64, -FMAX) < order_key(F64, -SUB) < order_key(F64, 0.0) < order_key(F64, SUB)
    assert order_key(F64, 2 ** 53) == order_key(F64, float(2 ** 53)) < order_key(F64, FMAX) < order_key(F64, float('inf'))
    assert order_key(CODE, 7) == 7


def test_rank_table_is_the_position_in_the_sorted_dictionary():
    words = ['b', 'a', 'é', '', 'B', 'aa']
    rank = rank_table(words)
    assert rank.dtype == np.int32 and rank.tolist() == [sorted(words).index(w) for w in words] == [4, 2, 5, 0, 1, 3]
    assert [words[i] for i in np.argsort(rank)] == sorted(words)
    assert rank_table(['only']).tolist() == [0] and rank_table([]).size == 0
    store = ColumnStore({'cat': str}, device='cpu')
    store.append([{'cat': w} for w in words] + [{}, None])
    assert rank_table(store.dictionary('cat')).tolist() == [4, 2, 5, 0, 1, 3]


def _store():
    store = ColumnStore([('n', int), ('price', float), ('cat', str)], device='cpu')
    store.append([{'n': i, 'price': i / 2, 'cat': 'ab'[i % 2]} for i in range(40)])
    return store


def test_page_leaves_these_calls_to_the_host():
    store = _store()
    assert store.page(None, 'extra', True, 0, 10) is None  # not declared
    for limit in (0, -1, PAGE_MAX + 1):
        assert store.page(None, 'n', True, 0, limit) is None and store.page(None, None, True, 0, limit) is None
    assert store.page(None, 'n', True, -1, 10) is None and store.page(None, None, True, -1, 10) is None
    assert store.page(None, 'n', True, 2 ** 31 - 10, 10) is None
    assert PAGE_MAX == 4096
    # an irregular column: a NaN; a str in an int column
    store.append([{'price': float('nan'), 'n': 1}])
    assert store.irregular == {'price'} and store.page(None, 'price', True, 0, 10) is None
    store.append([{'n': 'seven'}])
    assert store.irregular == {'price', 'n'} and store.page(None, 'n', False, 0, 10) is None
    # no rows
    empty = ColumnStore([('n', int)], device='cpu')
    assert empty.page(None, 'n', True, 0, 10) is None and empty.page(None, None, True, 0, 10) is None
    store.clear()
    assert store.page(None, 'cat', True, 0, 10) is None


def test_last_filter_page_without_columns(tmp_path):
    """an ``AnnLite`` without declared columns answers every page on the host"""
    from annlite_amd import AnnLite
    from annlite_amd.index import Document

    ann = AnnLite(64, n_subvectors=8, data_path=tmp_path / 'f')
    assert ann.last_filter_page is None
    for i in range(10):  # fill the in-memory table the way index() does
        d = Document(id=str(i), embedding=np.zeros(64, np.float32), tags={'price': 10 - i, 'cat': i % 3})
        ann._offset2id.append(d.id)
        ann._id2offset[d.id] = i
        ann._tags.append(dict(d.tags))
        ann._docs[d.id] = d
    assert [d.id for d in ann.filter({'cat': {'$eq': 1}}, limit=10)] == ['1', '4', '7']
    assert ann.last_filter_page == 'host'
    assert [d.id for d in ann.filter({'price': {'$gte': 5}}, limit=2, offset=1, order_by='price')] == ['4', '3']
    assert [d.id for d in ann.get_docs(limit=3)] == ['0', '1', '2'] and ann.last_filter_page == 'host'
