"""The argument checks of the 20 float-search entries of the C ABI: six searches, six filter stages, six workspace
sizes and the two readers of a workspace, over the four filters and the three kinds of row set.  A table of argument tuples, the return
code of each.  The library loads without a GPU and no pointer here is ever followed: every call is refused, or has nothing to do, or
-- where the point is that the checks ACCEPT it -- stops at a 16-byte workspace (the one entry without a workspace: at ``B = 0``)."""
import ctypes

import pytest

OK, INVALID, WORKSPACE = 0, 1, 4
FILTERS = ('f32', 'bf16x3', 'f16x2', 'i8x3')
INT32_MAX = 2 ** 31 - 1

_TABLE = {'f32': ('', 'norms N'), 'bf16x3': ('_split', 'norms N'), 'f16x2': ('_f16', 'norms N'), 'i8x3': ('_i8', 'scale norms N')}
_STAGE_OUT = {'bf16x3': 'qn_out bounds cand count centre scores', 'f16x2': 'qn_out qx_out bounds cand count scores',
              'i8x3': 'qn_out qx_out bounds cand count scores'}
_SET = {'rows': 'filter metric q B D x scale norms centre N rows n_sel', 'grouped': 'filter metric q B D x scale norms centre N valid masks ld G group'}


def _entries():
    """``{(job, kind, filter): (name, parameter names in order)}`` of the twelve search and stage entries, by what each row set takes"""
    e = {}
    for f, (suffix, mid) in _TABLE.items():
        centre = ' centre' if f == 'bf16x3' else ''
        e['search', 'table', f] = ('annlite_flat_search_topk' + suffix, f'metric q B D x {mid} valid{centre} k flags out_d out_i ws ws_bytes stream')
        if f == 'f32':
            e['stage', 'table', f] = ('annlite_flat_filter', 'metric q B D x norms N stride valid qnorms bounds cand count stream')
        else:
            e['stage', 'table', f] = ('annlite_flat_filter' + suffix, f'metric q B D x {mid} stride valid {_STAGE_OUT[f]} ws ws_bytes stream')
        for kind, head in _SET.items():
            e['search', kind, f] = (f'annlite_flat_search_topk_{kind}', head + ' k flags out_d out_i ws ws_bytes stream')
            e['stage', kind, f] = (f'annlite_flat_filter_{kind}', head + ' stride bounds cand count scores ws ws_bytes stream')
    return {key: (name, sig.split()) for key, (name, sig) in e.items()}


ENTRIES = _entries()
# every pointer a fake 8; a 16-byte workspace, so that a call the checks accept goes no further
DEFAULTS = dict(metric=1, q=8, B=4, D=8, x=8, scale=1.0, norms=8, centre=None, N=100, valid=None, rows=8, n_sel=50, masks=8, ld=4, G=2, group=8,
                k=10, flags=0, stride=1, out_d=8, out_i=8, bounds=8, cand=8, count=8, qnorms=8, qn_out=None, qx_out=None, scores=None, ws=8,
                ws_bytes=16, stream=None)
POINTERS = ('q', 'x', 'norms', 'rows', 'masks', 'group', 'out_d', 'out_i', 'bounds', 'cand', 'count', 'qnorms', 'ws')


@pytest.fixture(scope='module')
def capi():
    from annlite_amd import _capi

    return _capi, _capi.lib()


def _call(capi, key, **kw):
    """the entry ``key`` with ``kw`` over the defaults; None where the entry has no such parameter"""
    _capi, lib = capi
    name, params = ENTRIES[key]
    if not set(kw) <= set(params):
        return None
    assert 'ws_bytes' in params or kw, 'annlite_flat_filter launches what it accepts: never called with the defaults alone'
    vals = {**DEFAULTS, 'filter': _capi.FLAT_FILTER[key[2]], **kw}
    return getattr(lib, name)(*[vals[p] for p in params])


def _accepted(key):
    """what an entry returns for arguments its checks accept: the workspace code, or OK from the entry without a workspace (at B = 0)"""
    return WORKSPACE if 'ws_bytes' in ENTRIES[key][1] else OK


def _is(flt_set, then, otherwise):
    return lambda key: then if key[2] in flt_set else otherwise


# (what varies, the code -- a constant, or a function of (job, kind, filter) --, a word of the message or None)
CASES = [
    (dict(metric=0), INVALID, 'metric'),
    (dict(metric=4), INVALID, 'metric'),
    (dict(D=0), INVALID, 'shape'),
    (dict(D=40000, B=0), _is(('f32',), OK, INVALID), None),                 # D beyond the split filters' bound: the f32 filter takes it
    (dict(D=40000), lambda key: None if 'ws_bytes' not in ENTRIES[key][1] else WORKSPACE if key[2] == 'f32' else INVALID, None),
    (dict(B=-1), INVALID, 'shape'),
    (dict(B=INT32_MAX + 1), INVALID, 'shape'),
    (dict(N=-1, n_sel=0), INVALID, None),
    (dict(N=-1), INVALID, None),
    (dict(N=INT32_MAX + 1), INVALID, 'shape'),
    (dict(k=0), INVALID, 'k'),
    (dict(k=65), INVALID, 'k'),
    (dict(k=64), lambda key: _accepted(key), None),
    (dict(stride=0), INVALID, 'shape'),
    (dict(stride=-2), INVALID, 'shape'),
    (dict(n_sel=-1), INVALID, 'n_sel'),
    (dict(n_sel=101), INVALID, 'n_sel'),
    (dict(n_sel=100), lambda key: _accepted(key), None),
    (dict(G=0), INVALID, 'G'),
    (dict(G=-3), INVALID, 'G'),
    (dict(G=2 ** 32 + 1), INVALID, 'G'),                                      # (not narrowed to an int before the check)
    (dict(ld=3), INVALID, 'mask_ld'),                                         # 96 bits for 100 rows
    (dict(ld=-1), INVALID, 'mask_ld'),
    (dict(filter=4), INVALID, 'filter'),
    (dict(filter=-1), INVALID, 'filter'),
    (dict(centre=8), lambda key: _accepted(key) if key[2] == 'bf16x3' else INVALID, None),   # a centre is the split filter's ...
    (dict(centre=8, metric=2), INVALID, 'centre'),                            # ... and EUCLIDEAN's
    (dict(centre=8, metric=3), INVALID, 'centre'),
    (dict(centre=8, metric=2, B=0), INVALID, 'centre'),                       # (checked before "nothing to do")
    (dict(scale=3.0), lambda key: INVALID if key[2] == 'i8x3' else _accepted(key), None),    # int8 rows: a power of two; nobody else reads it
    (dict(scale=0.0), lambda key: INVALID if key[2] == 'i8x3' else _accepted(key), None),
    (dict(scale=3.0, B=0), _is(('i8x3',), INVALID, OK), None),
    (dict(scale=0.5), lambda key: _accepted(key), None),
    (dict(scores=8), lambda key: INVALID if key[2] == 'f32' else _accepted(key), None),      # (the f32 kernel has no scores)
    (dict(scores=8, B=0), _is(('f32',), INVALID, OK), None),
    (dict(ws_bytes=16), WORKSPACE, 'workspace'),
    (dict(ws_bytes=0), WORKSPACE, 'workspace'),
]
# nothing to do: OK with NULL everywhere, nothing is read.  (what varies, the kinds of row set it applies to, the code by job)
ALL_KINDS = ('table', 'rows', 'grouped')
STAGE_ONLY = {'stage': OK, 'search': INVALID}  # a search over no rows still writes B answers: its pointers are read
EARLY = [
    (dict(B=0), ALL_KINDS, {'stage': OK, 'search': OK}),
    (dict(B=0, N=0, n_sel=0), ALL_KINDS, {'stage': OK, 'search': OK}),
    (dict(N=0), ('table', 'grouped'), STAGE_ONLY),
    (dict(N=0, ld=0), ('grouped',), STAGE_ONLY),
    (dict(N=0, n_sel=0), ('rows',), STAGE_ONLY),
    (dict(n_sel=0), ('rows',), STAGE_ONLY),
    (dict(B=0, metric=0), ALL_KINDS, {'stage': INVALID, 'search': INVALID}),  # (the checks come first)
    (dict(B=0, D=0), ALL_KINDS, {'stage': INVALID, 'search': INVALID}),
]


def test_every_entry_returns_its_code(capi):
    err = lambda: capi[1].annlite_hip_last_error().decode()
    ran = [0] * len(CASES)
    for key in ENTRIES:
        for n, (kw, want, word) in enumerate(CASES):
            want = want(key) if callable(want) else want
            rc = None if want is None else _call(capi, key, **kw)
            if rc is None:
                continue  # (the entry has no such parameter)
            ran[n] += 1
            assert rc == want, (key, kw, rc, err())
            if word and rc == INVALID:
                assert word in err(), (key, kw, err())
    assert all(ran), [CASES[n][0] for n, r in enumerate(ran) if not r]


def test_nothing_to_do_reads_no_pointer(capi):
    ran = [0] * len(EARLY)
    for key, (name, params) in ENTRIES.items():
        for n, (kw, kinds, want) in enumerate(EARLY):
            if key[1] not in kinds:
                continue
            kw = {p: v for p, v in kw.items() if p in params or p != 'n_sel'}
            rc = _call(capi, key, **{p: None for p in POINTERS if p in params}, **kw)
            ran[n] += 1
            assert rc == want[key[0]], (key, kw, rc)
    assert all(ran)


def test_each_required_pointer_in_turn(capi):
    err = lambda: capi[1].annlite_hip_last_error().decode()
    for key, (name, params) in ENTRIES.items():
        required = [p for p in POINTERS if p in params]
        assert len(required) >= 6, key
        for p in required:
            assert _call(capi, key, **{p: None}) == INVALID and 'null' in err(), (key, p, err())
        # the list is required also where it is empty; the rows and their norms are not, in a search over no rows
        if key[1] == 'rows':
            assert _call(capi, key, rows=None, n_sel=0) == (INVALID if key[0] == 'search' else OK), key
        if key[0] == 'search':
            empty = dict(n_sel=0) if key[1] == 'rows' else dict(N=0, ld=0) if key[1] == 'grouped' else dict(N=0)
            assert _call(capi, key, x=None, norms=None, **empty) == WORKSPACE, key
            assert _call(capi, key, x=None) == INVALID and _call(capi, key, norms=None) == INVALID, key
        # what is optional: the live bitmap, and what a typed stage hands back
        for p in ('valid', 'qn_out', 'qx_out'):
            if p in params and 'ws_bytes' in params:
                assert _call(capi, key, **{p: 8}) == WORKSPACE, (key, p)


WS_ENTRIES = {'f32': 'annlite_flat_search_workspace_bytes', 'bf16x3': 'annlite_flat_search_split_workspace_bytes',
              'f16x2': 'annlite_flat_search_f16_workspace_bytes', 'i8x3': 'annlite_flat_search_i8_workspace_bytes'}
# (N, D, B, k) -> the typed entries' code by filter, the rows / grouped entries' code by filter
WS_CASES = [
    ((9000, 5, 130, 10), OK, OK),
    ((0, 33, 0, 1), OK, OK),
    ((100, 8, 4, 64), OK, OK),
    ((100, 0, 4, 10), INVALID, INVALID),
    ((100, 40000, 4, 10), _is(('f32',), OK, INVALID), _is(('f32',), OK, INVALID)),
    ((100, 32768, 4, 10), OK, OK),
    ((100, 32769, 4, 10), _is(('f32',), OK, INVALID), _is(('f32',), OK, INVALID)),
    ((100, 8, 4, 0), INVALID, INVALID),
    ((100, 8, 4, 65), INVALID, INVALID),
    ((-1, 8, 4, 10), INVALID, INVALID),
    ((100, 8, -1, 10), INVALID, INVALID),
    ((INT32_MAX + 1, 8, 4, 10), OK, INVALID),                                 # the typed entries never bounded N ...
    ((100, 8, INT32_MAX + 1, 10), OK, INVALID),                               # ... nor B
    ((100, INT32_MAX + 1, 4, 10), _is(('f32',), OK, INVALID), INVALID),      # ... nor the f32 filter's D
]


def test_the_workspace_entries(capi):
    _capi, lib = capi
    code_of = lambda want, f: want(('ws', '', f)) if callable(want) else want
    typed, other = ctypes.c_int64(0), ctypes.c_int64(0)
    for f in FILTERS:
        for (N, D, B, k), want_typed, want_set in WS_CASES:
            assert getattr(lib, WS_ENTRIES[f])(N, D, B, k, ctypes.byref(typed)) == code_of(want_typed, f), (f, N, D, B, k)
            for kind in ('rows', 'grouped'):
                rc = getattr(lib, f'annlite_flat_search_{kind}_workspace_bytes')(_capi.FLAT_FILTER[f], N, D, B, k, ctypes.byref(other))
                assert rc == code_of(want_set, f), (f, kind, N, D, B, k)
                if rc == OK and code_of(want_typed, f) == OK:
                    assert other.value == typed.value > 0, (f, kind, N, D, B, k)  # one workspace per filter, whatever the row set
        assert getattr(lib, WS_ENTRIES[f])(100, 8, 4, 10, None) == INVALID
    for kind in ('rows', 'grouped'):
        entry = getattr(lib, f'annlite_flat_search_{kind}_workspace_bytes')
        assert entry(0, 100, 8, 4, 10, None) == INVALID
        assert entry(4, 100, 8, 4, 10, ctypes.byref(other)) == INVALID and entry(-1, 100, 8, 4, 10, ctypes.byref(other)) == INVALID


def test_the_readers_of_a_workspace(capi):
    _capi, lib = capi
    n = ctypes.c_int64(0)
    assert lib.annlite_flat_overflow_count(None, None, ctypes.byref(n)) == INVALID
    assert lib.annlite_flat_overflow_count(8, None, None) == INVALID
    assert lib.annlite_flat_list_counts(None, 4, 8, None) == INVALID
    assert lib.annlite_flat_list_counts(8, 4, None, None) == INVALID
    assert lib.annlite_flat_list_counts(8, -1, 8, None) == INVALID
    assert lib.annlite_flat_list_counts(8, 0, 8, None) == OK
