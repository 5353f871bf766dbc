"""``annlite_filter_eval`` (filter.hip): the kernel's packed mask, unpacked, against ``filter.select`` over the
same tags -- at the row counts where a ballot of 64 rows into two words can go wrong, past one pass of a capped grid, with NULLs in
every column, dropped rows, the int64 extremes, the integers around 2^53, signed zeros, infinities and denormals."""
import numpy as np
import pytest

from conftest import has_gpu
from test_filter_compile_host import COLUMNS, P53, TAGS, _or_chain

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

FILTERS = [
    {'i': {'$gt': 0}},
    {'i': {'$lt': 2.5}, 'f': {'$gte': -0.0}},
    {'i': P53}, {'i': P53 + 1}, {'i': {'$gt': P53}}, {'i': {'$in': [P53 + 1, -P53 - 1, 3]}},
    {'i': {'$lte': -2 ** 63}}, {'i': {'$gte': 2 ** 63 - 1}}, {'i': {'$neq': 2 ** 63 - 1}}, {'i': {'$nin': [0, 1]}},
    {'f': 0.0}, {'f': {'$lt': 0.0}}, {'f': {'$lt': 5e-324}}, {'f': {'$gt': -5e-324, '$lt': 2.2250738585072014e-308}},
    {'f': {'$lt': float('inf')}}, {'f': float('-inf')}, {'f': {'$in': [2, 2.5, float('inf')]}}, {'f': {'$neq': 2.5}},
    {'s': 'red'}, {'s': {'$in': 'abcd'}}, {'s': {'$lt': 'b'}}, {'s': {'$neq': 'red'}},
    {'b': True},
    {'$or': {'i': {'$lt': -1}, '$and': {'f': {'$gt': 0.0}, 's': {'$nin': ['red', 'blue']}}}},
    {'$not': {'i': {'$gt': 0}}}, {'s': 'red', '$not': {'f': {'$lt': 1.0}}},
    {'$and': {}},
    {'$or': [{'i': {'$lt': j - 16}} for j in range(32)]},   # 32 leaves
    _or_chain(32),                                           # a stack of 32
]


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _store(tags, **kw):
    from annlite_amd.columns import ColumnStore

    st = ColumnStore(COLUMNS, **kw)
    st.append(tags)
    return st


def _unpack(words):
    w = words.cpu().numpy().view(np.uint32)
    return ((w[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1).astype(bool).reshape(-1)


def _check(st, tags, flt, max_blocks=0):
    from annlite_amd.filter import select

    prog = st.compile(flt)
    assert prog is not None, flt
    mask = st.evaluate(prog, max_blocks=max_blocks)
    want = select(tags, flt)
    bits = _unpack(mask.words)
    n = len(tags)
    assert mask.words.numel() == (st.capacity + 31) // 32 + 2 and bits.size >= n + 64
    assert np.flatnonzero(bits).tolist() == want, (flt, n)  # (no bit at or behind row n: every word there is 0, the pads included)
    assert len(mask) == len(want) == int(bits.sum())        # the counter is the popcount
    assert mask.offsets().tolist() == want and mask.offsets().dtype == np.int64
    return mask


@pytest.mark.parametrize('n', [1, 31, 32, 33, 63, 64, 65, 257])
def test_mask_equals_select_at_the_word_and_wave_edges(ops, n):
    tags = TAGS[-n:] if n <= len(TAGS) else TAGS
    tags = list(tags[:n])
    st = _store(tags, initial_capacity=64)
    for flt in FILTERS:
        _check(st, tags, flt)


def test_rows_past_one_pass_of_a_capped_grid(ops):
    tags = (TAGS * 3)[:2 * 256 + 1]
    st = _store(tags, initial_capacity=64)
    for flt in FILTERS[:8] + FILTERS[-3:]:
        _check(st, tags, flt, max_blocks=2)   # 513 rows, 2 workgroups of 256: the last row is the second pass
        _check(st, tags, flt, max_blocks=1)
    _check(st, tags, FILTERS[0], max_blocks=3)


def test_capacity_beyond_the_rows_every_word_written(ops):
    import torch
    from annlite_amd.filter import select

    tags = list(TAGS[:100])
    st = _store(tags, initial_capacity=4096)
    assert st.capacity == 4096 and st.n_words == 130
    for flt in ({'$and': {}}, {'i': {'$gt': 0}}, {'$not': {'i': {'$gt': 0}}}):  # (TRUE and NOT would set the rows behind N if they were evaluated)
        P, keep = st.bind(st.compile(flt))
        out = torch.full((st.n_words,), -1, dtype=torch.int32, device=st.rows.device)
        for and_bits in (st.rows, None, torch.full_like(st.rows, -1)):
            out.fill_(-1)
            _, count = ops.filter_eval(P, len(st), st.n_words, and_bits=and_bits, out=out)
            bits = _unpack(out)
            want = select(tags, flt) if and_bits is st.rows else select([t if t is not None else {} for t in tags], flt)
            assert np.flatnonzero(bits).tolist() == want and int(count.item()) == len(want)
            assert (out[4:] == 0).all()  # words 4 .. 129: rows 128 .. and the two pads


def test_and_bits_and_the_counter(ops):
    import torch
    from annlite_amd.filter import select

    tags = list(TAGS)
    st = _store(tags)
    rs = np.random.RandomState(3)
    keep_rows = rs.rand(len(tags)) < 0.5
    flags = np.zeros(st.n_words * 32, dtype=bool)
    flags[:len(tags)] = keep_rows
    flags[len(tags):] = True  # (bits behind the rows in the caller's words do not come through)
    and_bits = torch.from_numpy(np.packbits(flags, bitorder='little').view(np.int32)).to(st.rows.device)
    flt = {'i': {'$gte': 0}}
    P, keep = st.bind(st.compile(flt))
    count = torch.full((1,), 1000, dtype=torch.int64, device=st.rows.device)
    out, count = ops.filter_eval(P, len(st), st.n_words, and_bits=and_bits, count=count)
    want = [o for o in select([t or {} for t in tags], flt) if keep_rows[o]]
    assert np.flatnonzero(_unpack(out)).tolist() == want
    assert int(count.item()) == 1000 + len(want)  # ADDED to the caller's counter


def test_dropped_rows_and_growth_keep_the_answer(ops):
    tags = list(TAGS[:50])
    st = _store(tags, initial_capacity=64)
    assert st.capacity == 64
    _check(st, tags, {'i': {'$gt': 0}})
    st.append(TAGS[50:70])   # grows
    tags += TAGS[50:70]
    assert st.capacity > 64
    st.append(TAGS[70:])     # grows again
    tags += TAGS[70:]
    for flt in FILTERS:
        _check(st, tags, flt)
    gone = [0, 31, 32, 33, 63, 64, 65, 200, 259]
    st.drop(gone)
    for o in gone:
        tags[o] = None
    for flt in FILTERS:
        _check(st, tags, flt)
    st.clear()
    assert len(st) == 0 and st.capacity == 0
    st.append(TAGS[:5])
    _check(st, list(TAGS[:5]), {'$and': {}})


def test_programs_beyond_a_limit_do_not_compile_and_bad_programs_are_refused(ops):
    from annlite_amd import _capi
    from annlite_amd.columns import CODE_AND, CODE_NOT, CODE_TRUE

    st = _store(list(TAGS))
    assert st.compile({'$or': [{'i': {'$lt': j - 16}} for j in range(33)]}) is None
    deep = {'i': 1}
    for _ in range(32):
        deep = {'$or': [[], deep]}
    assert st.compile(deep) is None
    good = st.compile({'i': {'$gt': 0}, 'f': {'$lt': 1.0}})

    def refused(change):
        P, keep = st.bind(good)
        change(P)
        with pytest.raises(AssertionError):
            ops.filter_eval(P, len(st), st.n_words, and_bits=st.rows)

    def code(*ops_):
        def change(P):
            P.n_code = len(ops_)
            for j, o in enumerate(ops_):
                P.code[j] = o
        return change

    refused(code(0, CODE_AND))                 # underflow
    refused(code(0, 1))                        # two values left
    refused(code(CODE_NOT))                    # NOT on nothing
    refused(code(2))                           # a leaf the program does not have
    refused(code(0x90))                        # unknown op
    refused(code(*([CODE_TRUE] * 33 + [CODE_AND] * 32)))  # a stack of 33
    refused(lambda P: setattr(P, 'n_leaves', 33))
    refused(lambda P: setattr(P, 'n_literals', 65))
    refused(lambda P: setattr(P, 'n_code', 0))
    refused(lambda P: setattr(P.leaves[0], 'lit_begin', 2))   # literals [2, 3) of 2
    refused(lambda P: setattr(P.leaves[0], 'kind', 7))
    refused(lambda P: setattr(P.leaves[1], 'values_dev', None))
    P, keep = st.bind(good)
    with pytest.raises(AssertionError):
        ops.filter_eval(P, len(st), (len(st) + 31) // 32 - 1, and_bits=st.rows)  # fewer words than rows
    assert _capi.FILTER_MAX_LEAVES == 32 and _capi.FILTER_MAX_STACK == 32 and _capi.FILTER_MAX_LITERALS == 64
