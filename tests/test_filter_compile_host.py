"""CPU, no library: the filter compiler (annlite_amd/columns.py) against ``filter.select``.

A compiled program is run by the small numpy interpreter below over columns the store built on 'cpu' with its own type rule; the rows
it selects must be the rows ``filter.select`` selects over the same tags -- for every grammar form of filter.py's docstring, every row
of the lowering table at both sides of a boundary, the integers around 2^53, strings, and every rule that hands a filter back to
the host.
"""
import math

import numpy as np
import pytest

from annlite_amd import columns as C
from annlite_amd.columns import ColumnStore
from annlite_amd.filter import select

COLUMNS = [('i', int), ('f', float), ('s', str), ('b', bool)]
P53 = 2 ** 53


def _tags():
    ints = [C.INT64_MIN, C.INT64_MIN + 1, -P53 - 1, -P53, -3, -2, -1, 0, 1, 2, 3, 4, 5, P53 - 1, P53, P53 + 1, C.INT64_MAX - 1, C.INT64_MAX,
            True, False, np.int32(7), np.int64(-7)]
    floats = [-math.inf, -1e300, -2.5, -2.0, -5e-324, -0.0, 0.0, 5e-324, 2.2250738585072014e-308, 2.0, 2.5, 3.0, 3.5, 1e300, math.inf,
              3, -2, P53, -P53, np.float64(2.5)]
    words = ['', 'a', 'ab', 'abc', 'b', 'ba', 'red', 'green', 'blue', 'Red']
    rs = np.random.RandomState(5)
    tags = []
    for r in range(260):
        t = {}
        if r % 7 != 3:
            t['i'] = ints[r % len(ints)] if r < 2 * len(ints) else int(rs.randint(-6, 7))
        if r % 5 != 1:
            t['f'] = floats[(r * 3) % len(floats)] if r < 3 * len(floats) else float(rs.randint(-8, 9)) / 2
        if r % 6 != 2:
            t['s'] = words[int(rs.randint(len(words)))]
        if r % 4 == 0:
            t['b'] = bool(r % 8)
        if r % 3 == 0:
            t['u'] = r  # (a tag that is not declared)
        if r % 11 == 10:
            t['f'] = None  # (an explicit None is a NULL like a missing tag)
        tags.append(None if r % 29 == 17 else t)  # (None: a deleted document's row)
    tags[40] = {}
    return tags


TAGS = _tags()


def _store(tags=TAGS, columns=COLUMNS, **kw):
    st = ColumnStore(columns, device='cpu', **kw)
    st.append(tags)
    return st


STORE = _store()


def _bits(words, n):
    w = words.numpy().view(np.uint32)
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(-1)[:n]


def interpret(prog, store):
    """the program as the kernel runs it, in numpy: a leaf is present & compare in the column's own type; postfix over a stack"""
    n = len(store)
    leaves = []
    for leaf in prog.leaves:
        x = store.values[leaf.column].numpy()[:n]
        assert x.dtype == {C.I64: np.int64, C.F64: np.float64, C.CODE: np.int32}[leaf.kind]
        lits = prog.literals[leaf.lit_begin: leaf.lit_begin + leaf.lit_count]
        assert all(type(v) is (float if leaf.kind == C.F64 else int) for v in lits)
        if leaf.op == C.OP_IN_SET:
            r = _bits(__import__('torch').from_numpy(leaf.set_bits.view(np.int32)), leaf.set_bits.size * 32)[x]
        elif leaf.op in (C.OP_IN, C.OP_NIN):
            r = np.zeros(n, dtype=bool)
            for v in lits:
                r |= x == v
            r = r if leaf.op == C.OP_IN else ~r
        else:
            (v,) = lits
            r = {C.OP_LT: x < v, C.OP_GT: x > v, C.OP_LE: x <= v, C.OP_GE: x >= v, C.OP_EQ: x == v, C.OP_NE: x != v}[leaf.op]
        leaves.append(r & _bits(store.present[leaf.column], n))
    stack, deepest = [], 0
    for op in prog.code:
        if op < 32:
            stack.append(leaves[op])
        elif op == C.CODE_TRUE:
            stack.append(np.ones(n, dtype=bool))
        elif op == C.CODE_NOT:
            stack.append(~stack.pop())
        else:
            b, a = stack.pop(), stack.pop()
            stack.append(a & b if op == C.CODE_AND else a | b)
        deepest = max(deepest, len(stack))
    assert len(stack) == 1 and deepest == prog.depth <= C.MAX_STACK
    assert len(prog.leaves) <= C.MAX_LEAVES and len(prog.literals) <= C.MAX_LITERALS and len(prog.code) <= C.MAX_CODE
    return np.nonzero(stack[0] & _bits(store.rows, n))[0].tolist()


def check(flt, store=STORE, tags=TAGS):
    prog = store.compile(flt)
    assert prog is not None, flt
    got, want = interpret(prog, store), select(tags, flt)
    assert got == want, (flt, sorted(set(got) ^ set(want))[:8])
    return prog, want


GRAMMAR = [
    {'i': {'$lt': 3}},
    {'i': {'$gt': -2, '$lte': 3}},                                   # several operators on one field
    {'i': {'$gte': 0}, 'f': {'$lt': 2.5}},                           # two fields: AND
    {'$and': {'i': {'$gt': 0}, 'f': {'$lte': 3.0}}},
    {'$or': {'i': {'$lt': -1}, 'f': {'$gt': 3.0}}},
    {'$and': {'i': {'$gt': 0}, '$or': {'f': {'$lt': 0.0}, 's': 'red'}}},   # $or as the 2nd key of an AND clause: joined by OR
    {'$or': {'i': {'$gt': 3}, '$and': {'f': {'$lt': 0.0}, 's': {'$neq': 'red'}}}},  # $and as the 2nd key of an OR clause
    {'i': {'$lt': 0}, '$or': {'f': {'$gt': 2.0}, 's': 'blue'}},      # a OR f OR s?  no: i AND? -- the splice decides, select is the judge
    {'s': 'red', '$and': {'i': {'$gt': 0}, 'f': {'$gt': 0.0}}},
    {'$or': [{'i': {'$lt': -2}}, [{'f': {'$gt': 0.0}}, {'s': {'$in': ['red', 'blue']}}]]},  # a list group inside an OR
    {'$or': [{'i': 1, 'f': {'$gt': 0.0}}, {'s': 'green'}]},
    {'$and': [{'$or': {'i': 1, 's': 'a'}}, {'f': {'$gte': 0.0}}]},
    [{'i': {'$gt': 0}}, {'f': {'$lt': 1.0}}],                        # a list at the top
    {'$not': {'i': {'$gt': 0}}},
    {'s': 'red', '$not': {'i': {'$lt': 0}, 'f': {'$gt': 0.0}}},
    {'$or': {'i': 2, '$not': {'s': {'$in': ['red', 'green']}}}},
    {'$not': {'$not': {'i': {'$neq': 1}}}},
    {'i': {'$in': [1, 2, 5, C.INT64_MAX]}},
    {'i': {'$nin': [0, 1, -1]}},
    {'i': {'$in': []}},
    {'i': {'$nin': []}},
    {'f': {'$in': (2.5, -0.0, math.inf)}},
    {'i': {'$in': {3, 4}}},
    {'i': 3},                                                        # bare equality
    {'s': 'abc'},
    {'b': True},
    {'b': {'$ne': True}},
    {'i': {'$ne': 3}},
    {'i': {'$neq': 3}},
    {'f': {'$ne': 0.0}},
    {'$and': {}},                                                    # an empty {} under $and: everything
    {'i': {'$gt': 0}, '$and': {}},
    {'$or': {}},
    {'i': {'$gt': 0}, '$or': {}},
    {'i': {'$and': {'f': {'$gt': 0.0}, 's': 'red'}}},                # a logical operator under a field
    {'i': {'$gt': 0, '$or': {'f': {'$lt': 0.0}, 's': 'red'}}},
    {'$or': [[], {'i': 1}]},
]


@pytest.mark.parametrize('flt', GRAMMAR, ids=[str(i) for i in range(len(GRAMMAR))])
def test_grammar_forms_select_the_same_rows(flt):
    check(flt)


def test_the_corpus_is_not_trivial():
    n_live = len(select(TAGS, {}))
    sizes = [len(select(TAGS, f)) for f in GRAMMAR]
    assert sum(0 < s < n_live for s in sizes) >= 25


LOWERING = [('$lt', 2.5), ('$lt', 3.0), ('$lte', 2.5), ('$lte', -2.5), ('$lte', 3.0), ('$gt', 2.5), ('$gt', -2.5), ('$gt', 3.0), ('$gte', 2.5),
            ('$gte', -2.5), ('$gte', 3.0), ('$lt', -2.5), ('$eq', 3.0), ('$eq', 3.5), ('$neq', 3.0), ('$neq', 3.5), ('$eq', -0.0),
            ('$lt', math.inf), ('$lte', math.inf), ('$gt', math.inf), ('$gte', math.inf), ('$eq', math.inf), ('$neq', math.inf),
            ('$lt', -math.inf), ('$lte', -math.inf), ('$gt', -math.inf), ('$gte', -math.inf), ('$eq', -math.inf), ('$neq', -math.inf),
            ('$lt', 1e30), ('$gt', 1e30), ('$lte', -1e30), ('$gte', -1e30), ('$eq', 1e30), ('$neq', -1e30),
            ('$lt', 2.0 ** 63), ('$gte', 2.0 ** 63), ('$gte', -2.0 ** 63), ('$lt', -2.0 ** 63), ('$eq', 2.0 ** 63), ('$eq', -2.0 ** 63),
            ('$gt', float(P53)), ('$gte', float(P53)), ('$eq', float(P53)), ('$lt', float(P53)), ('$lte', float(P53)),
            ('$in', [3.0, 3.5, 2, math.inf, 1e30]), ('$nin', [3.0, 3.5, -2.0])]


@pytest.mark.parametrize('op,c', LOWERING, ids=['%s %r' % oc for oc in LOWERING])
def test_int_column_against_a_float_literal(op, c):
    prog, _ = check({'i': {op: c}})
    assert all(type(v) is int and C.INT64_MIN <= v <= C.INT64_MAX for v in prog.literals)


def test_lowering_table():
    L = C._lower_i64
    assert L(C.OP_LT, 2.5) == (C.OP_LT, 3) and L(C.OP_LE, 2.5) == (C.OP_LE, 2) and L(C.OP_GT, 2.5) == (C.OP_GT, 2) and L(C.OP_GE, 2.5) == (C.OP_GE, 3)
    assert L(C.OP_LT, -2.5) == (C.OP_LT, -2) and L(C.OP_LE, -2.5) == (C.OP_LE, -3) and L(C.OP_GT, -2.5) == (C.OP_GT, -3)
    assert L(C.OP_LT, 3.0) == (C.OP_LT, 3) and L(C.OP_EQ, 3.0) == (C.OP_EQ, 3) and L(C.OP_NE, 3.0) == (C.OP_NE, 3)
    assert L(C.OP_EQ, 3.5) == C._NEVER and L(C.OP_NE, 3.5) == C._ALWAYS
    assert L(C.OP_LT, math.inf) == C._ALWAYS and L(C.OP_GT, math.inf) == C._NEVER and L(C.OP_LT, -math.inf) == C._NEVER


@pytest.mark.parametrize('flt', [
    {'i': P53}, {'i': P53 + 1}, {'i': {'$gt': P53}}, {'i': {'$gte': P53 + 1}}, {'i': {'$lt': P53 + 1}}, {'i': {'$lte': -P53 - 1}},
    {'i': {'$in': [P53, -P53 - 1]}}, {'i': {'$nin': [P53 + 1]}}, {'i': C.INT64_MAX}, {'i': {'$gt': C.INT64_MIN}}, {'i': {'$lt': C.INT64_MIN}},
    {'i': {'$gt': C.INT64_MAX}}, {'i': {'$lte': C.INT64_MAX}}, {'i': True}, {'i': {'$gt': False}},
], ids=str)
def test_int_literals_around_2_to_53_and_the_extremes(flt):
    _, want = check(flt)
    if flt in ({'i': P53}, {'i': P53 + 1}):
        assert len(want) >= 1  # (adjacent integers a detour through f64 would merge)


@pytest.mark.parametrize('flt', [
    {'f': 3}, {'f': {'$gte': 2}}, {'f': {'$lt': -2}}, {'f': {'$in': [2, 2.5, -2]}}, {'f': {'$nin': [3]}}, {'f': P53}, {'f': {'$gt': -P53}}, {'f': True},
    {'f': 0.0}, {'f': -0.0}, {'f': {'$gt': 0.0}}, {'f': {'$lt': 5e-324}}, {'f': {'$gte': 5e-324}}, {'f': {'$lt': math.inf}}, {'f': math.inf},
    {'f': {'$gt': -math.inf}}, {'f': {'$lte': -math.inf}}, {'f': {'$lt': 2.2250738585072014e-308}}, {'f': {'$neq': -0.0}},
], ids=str)
def test_float_column(flt):
    check(flt)


@pytest.mark.parametrize('flt', [
    {'s': {'$lt': 'b'}}, {'s': {'$gte': 'ab'}}, {'s': {'$gt': ''}}, {'s': {'$in': 'abcd'}}, {'s': {'$nin': 'abcd'}}, {'s': {'$in': ['red', 'Red', 'x']}},
    {'s': {'$nin': ['red']}}, {'s': {'$neq': 'red'}}, {'s': {'$lt': 3}}, {'s': 3}, {'s': {'$neq': 3}}, {'s': {'$in': 5}}, {'s': {'$in': [1, 'a']}},
    {'s': {'$lte': 'red', '$gt': 'a'}},
], ids=str)
def test_string_column_has_pythons_semantics(flt):
    prog, _ = check(flt)
    assert all(leaf.op == C.OP_IN_SET for leaf in prog.leaves)


def test_type_rule_at_append():
    st = _store([{'i': True, 'f': 2, 's': 'x'}, {'i': np.int16(-4), 'f': np.float64(1.5)}, {'i': None}, None, {'f': False, 'i': np.int64(P53)}])
    assert not st.irregular and len(st) == 5
    assert st.values['i'][:5].tolist() == [1, -4, 0, 0, P53] and _bits(st.present['i'], 5).tolist() == [True, True, False, False, True]
    assert st.values['f'][:5].tolist() == [2.0, 1.5, 0.0, 0.0, 0.0] and _bits(st.present['f'], 5).tolist() == [True, True, False, False, True]
    assert _bits(st.rows, 5).tolist() == [True, True, True, False, True] and st.dictionary('s') == ['x']
    # every word behind the rows is 0, the two pads included
    assert st.rows.numel() == (st.capacity + 31) // 32 + 2 and st.rows[1:].abs().sum() == 0


IRREGULAR = [('i', 2.0), ('i', 'x'), ('i', 2 ** 63), ('i', -2 ** 63 - 1), ('i', np.int64(P53 + 1)), ('i', np.uint64(2 ** 63)), ('i', np.bool_(True)),
             ('f', math.nan), ('f', 'x'), ('f', P53 + 1), ('f', np.float32(1.5)), ('f', 1 + 2j), ('s', 3), ('s', b'x'), ('b', 0.5)]


@pytest.mark.parametrize('name,value', IRREGULAR, ids=['%s=%r' % nv for nv in IRREGULAR])
def test_a_value_outside_the_type_rule_makes_the_column_irregular(name, value):
    tags = [{'i': 1, 'f': 1.0, 's': 'a', 'b': True}, {name: value}, {'i': 2, 'f': 2.0, 's': 'b', 'b': False}]
    st = _store(tags)
    assert st.irregular == {name}
    assert st.compile({name: {'$neq': 0}}) is None and st.compile({'$or': {'s' if name != 's' else 'i': 'a', name: 1}}) is None
    other = next(n for n in ('i', 'f') if n != name)
    check({other: {'$gte': 1}}, st, tags)  # (the other columns still compile, over all three rows)
    st.append([{name: 1}])
    assert st.irregular == {name}  # ... until clear()
    st.clear()
    assert not st.irregular and len(st) == 0 and st.capacity == 0


def test_the_65537th_string_makes_the_column_irregular():
    tags = [{'s': 'w%d' % r, 'i': r} for r in range(C.MAX_STRINGS)]
    st = _store(tags, [('s', str), ('i', int)])
    assert not st.irregular and st.compile({'s': 'w7'}) is not None
    st.append([{'s': 'w7', 'i': 1}])  # (a known word: still regular)
    assert not st.irregular
    st.append([{'s': 'one more', 'i': 2}])
    assert st.irregular == {'s'} and st.compile({'s': 'w7'}) is None and st.compile({'i': 2}) is not None


UNCOMPILED = [
    {'u': 3},                                       # a field that is not declared
    {'i': 1, 'nope': {'$gt': 0}},
    {'i': math.nan}, {'f': {'$lt': math.nan}}, {'i': {'$in': [1, math.nan]}},
    {'i': 'x'}, {'f': {'$gt': 'x'}}, {'i': None}, {'i': {'$in': [1, 'x']}}, {'i': [1, 2]},
    {'i': 2 ** 63}, {'i': {'$lt': -2 ** 63 - 1}}, {'i': {'$in': [2 ** 63]}},
    {'f': P53 + 1}, {'f': {'$in': [1, -P53 - 1]}},
    {'i': np.int64(3)}, {'i': np.float64(2.5)}, {'f': np.float32(2.5)},   # numpy scalars as literals: numpy's comparison rules
    {'i': {'$in': 5}}, {'i': {'$in': 'abc'}}, {'i': {'$nin': {1: 2}}}, {'i': {'$in': np.array([1, 2])}},
]


@pytest.mark.parametrize('flt', UNCOMPILED, ids=str)
def test_filters_the_host_keeps(flt):
    assert STORE.compile(flt) is None


def _or_chain(n, leaf=lambda j: {'i': {'$lt': j}}):
    """OR(leaf_n, (OR(leaf_n-1, ( ... )))): n leaves, a stack of n"""
    flt = leaf(1)
    for j in range(2, n + 1):
        flt = {'$or': [leaf(j), flt]}
    return flt


def test_limits_are_conditions():
    prog, _ = check({'$or': [{'i': {'$lt': j - 16}} for j in range(32)]})
    assert len(prog.leaves) == 32 and prog.depth == 2
    assert STORE.compile({'$or': [{'i': {'$lt': j - 16}} for j in range(33)]}) is None
    prog, _ = check(_or_chain(32))
    assert prog.depth == 32 and len(prog.leaves) == 32
    flt = {'i': 1}
    for _ in range(32):
        flt = {'$or': [[], flt]}  # (TRUE pushes: a stack of 33 with one leaf)
    assert STORE.compile(flt) is None
    prog, _ = check({'i': {'$in': list(range(64))}})
    assert len(prog.literals) == 64
    assert STORE.compile({'i': {'$in': list(range(65))}}) is None
    assert STORE.compile({'i': {'$in': list(range(40))}, 'f': {'$in': [j / 2 for j in range(25)]}}) is None
    flt = {'i': 1}
    for _ in range(126):
        flt = {'$not': flt}
    prog, _ = check(flt)
    assert len(prog.code) == 127
    assert STORE.compile({'$not': {'$not': flt}}) is None  # (129 bytes of code)


MALFORMED = [{'$foo': 1}, {'i': {'$bar': 1}}, {'i': {}}, 5, 'i', {'$and': 5}, {'$or': [3]}, {'$not': 4}, {'i': 1, '$xor': {}}, {'i': {'$gt': 1, '$like': 'x'}},
             {'u': {'$bar': 1}}, {'u': 1, 'i': {}}, {'$not': {'$nope': 1}}]


@pytest.mark.parametrize('flt', MALFORMED, ids=str)
def test_the_same_exceptions_as_select(flt):
    with pytest.raises(ValueError) as want:
        select(TAGS, flt)
    for store in (STORE, ColumnStore(COLUMNS, device='cpu')):  # (on an empty table too)
        with pytest.raises(ValueError) as got:
            store.compile(flt)
        assert str(got.value) == str(want.value)
    with pytest.raises(ValueError):
        select([], flt)


def test_append_grows_and_keeps_old_rows_and_drop_clears_row_bits():
    st = ColumnStore(COLUMNS, device='cpu', initial_capacity=64)
    assert st.capacity == 0 and st.rows is None  # (nothing allocated before the first rows arrive)
    st.append(TAGS[:50])
    assert st.capacity == 64
    st.append(TAGS[50:70])
    cap = st.capacity
    assert cap >= 70
    st.append(TAGS[70:])
    assert st.capacity > cap and len(st) == len(TAGS)
    for name in ('i', 'f', 's'):
        n = len(TAGS)
        assert np.array_equal(st.values[name].numpy()[:n], STORE.values[name].numpy()[:n])
        assert np.array_equal(_bits(st.present[name], n), _bits(STORE.present[name], n))
    tags = list(TAGS)
    for flt in ({'i': {'$gt': 0}}, {'s': {'$in': 'abcd'}, 'f': {'$lt': 2.5}}):
        check(flt, st, tags)
    gone = [0, 31, 32, 33, 64, 200, 259, 259, 10 ** 6]
    st.drop(gone)
    for o in gone[:-1]:
        tags[o] = None
    for flt in ({'i': {'$gt': 0}}, {'$and': {}}):
        check(flt, st, tags)
