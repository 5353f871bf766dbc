"""The argument checks of the ten cells entries of the C ABI: three searches, two filter stages, two wide searches
and three workspace sizes, over the three cell-tile filters.  A table of argument tuples, the return code of each.  The library loads
without a GPU and no pointer here is ever followed: every call is refused, or has nothing to do, or -- where the point is that the checks
ACCEPT it -- stops at a 16-byte workspace.  The wide entries have no workspace: there "accepted" is a call with NULL queries that gets as
far as the pointer check, which comes behind every other check and behind "nothing to do"."""
import ctypes

import pytest

OK, INVALID, WORKSPACE = 0, 1, 4
ACCEPTED = WORKSPACE  # (read by _call for the wide entries as said above)
FILTERS = ('f32', 'bf16x3', 'f16x2')
INT32_MAX = 2 ** 31 - 1

_HEAD = 'metric q B D x norms N valid cells P C perm n_perm cell_rows cell_order max_cell_rows'
_SEARCH_TAIL = 'k flags out_d out_i ws ws_bytes stream'
_WIDE = 'metric q B D x N valid cells P C perm n_perm cell_rows k flags out_d out_i stream'
ENTRIES = {key: (name, sig.split()) for key, (name, sig) in {
    ('search', 'f32'): ('annlite_ivf_flat_search_topk', f'{_HEAD} max_probed_rows {_SEARCH_TAIL}'),
    ('search', 'bf16x3'): ('annlite_ivf_flat_search_topk_split', f'{_HEAD} max_probed_rows centres cell_of {_SEARCH_TAIL}'),
    ('search', 'f16x2'): ('annlite_ivf_flat_search_topk_f16', f'{_HEAD} max_probed_rows {_SEARCH_TAIL}'),
    ('stage', 'bf16x3'): ('annlite_ivf_flat_filter_split', f'{_HEAD} stride centres cell_of bounds cand count pn_out scores ws ws_bytes stream'),
    ('stage', 'f16x2'): ('annlite_ivf_flat_filter_f16', f'{_HEAD} stride qn_out qx_out bounds cand count scores ws ws_bytes stream'),
    ('wide', 'f32'): ('annlite_ivf_flat_search_topk_wide', _WIDE),
    ('wide', 'f16x2'): ('annlite_ivf_flat_search_topk_wide_f16', _WIDE),
}.items()}
# every pointer a fake 8; a 16-byte workspace, so that a call the checks accept goes no further
DEFAULTS = dict(metric=1, q=8, B=4, D=8, x=8, norms=8, N=100, valid=None, cells=8, P=2, C=16, perm=8, n_perm=50, cell_rows=8, cell_order=8,
                max_cell_rows=20, max_probed_rows=40, stride=1, centres=None, cell_of=None, k=None, flags=0, out_d=8, out_i=8, bounds=8,
                cand=8, count=8, pn_out=None, qn_out=None, qx_out=None, scores=None, ws=8, ws_bytes=16, stream=None)
POINTERS = ('q', 'x', 'norms', 'cells', 'perm', 'cell_rows', 'cell_order', 'out_d', 'out_i', 'bounds', 'cand', 'count', 'ws')


@pytest.fixture(scope='module')
def capi():
    from annlite_amd import _capi

    return _capi, _capi.lib()


def _err(capi):
    return capi[1].annlite_hip_last_error().decode()


def _raw(capi, key, **kw):
    name, params = ENTRIES[key]
    vals = {**DEFAULTS, **kw}
    if vals['k'] is None:
        vals['k'] = 100 if key[0] == 'wide' else 10
    if key[0] == 'wide':
        assert vals['B'] <= 0 or not all(vals[p] for p in ('q', 'x', 'perm', 'cells', 'cell_rows', 'out_d', 'out_i')), 'it would launch'
    return getattr(capi[1], name)(*[vals[p] for p in params])


def _call(capi, key, **kw):
    """the code of the entry ``key`` for ``kw`` over the defaults; None where the entry has no such parameter.  A wide entry is called with
    NULL queries: refused for that pointer, it returns ACCEPTED here."""
    if not set(kw) <= set(ENTRIES[key][1]):
        return None
    if key[0] != 'wide':
        return _raw(capi, key, **kw)
    rc = _raw(capi, key, q=None, **kw)
    return ACCEPTED if rc == INVALID and 'null' in _err(capi) else rc


def _is(keys, then, otherwise):
    return lambda key: then if key in keys or key[0] in keys or key[1] in keys else otherwise


F32_ROWS = (('search', 'f32'), ('wide', 'f32'))  # the entries without the split filters' bound on D
BOUND_P = (('search', 'f32'), ('wide', 'f32'), ('wide', 'f16x2'))  # the entries that bound P where the others bound B * P
# (what varies, the code -- a constant, or a function of (job, filter) --, a word of the message or None)
CASES = [
    (dict(), ACCEPTED, None),
    (dict(metric=0), INVALID, 'metric'),
    (dict(metric=4), INVALID, 'metric'),
    (dict(metric=2), ACCEPTED, None),
    (dict(metric=3), ACCEPTED, None),
    (dict(D=0), INVALID, 'shape'),
    (dict(D=32768), ACCEPTED, None),
    (dict(D=32769), _is(F32_ROWS, ACCEPTED, INVALID), 'shape'),
    (dict(D=32769, B=0), _is(F32_ROWS, OK, INVALID), 'shape'),
    (dict(B=-1), INVALID, 'shape'),
    (dict(B=INT32_MAX + 1, P=1), INVALID, 'shape'),
    (dict(N=-1, n_perm=0, max_cell_rows=0), INVALID, 'shape'),
    (dict(N=2 ** 31), INVALID, 'shape'),
    (dict(N=INT32_MAX, n_perm=INT32_MAX, max_cell_rows=INT32_MAX), ACCEPTED, None),
    (dict(k=0), INVALID, 'k'),
    (dict(k=1), _is(('wide',), INVALID, ACCEPTED), 'k'),
    (dict(k=64), _is(('wide',), INVALID, ACCEPTED), 'k'),
    (dict(k=65), _is(('wide',), ACCEPTED, INVALID), 'k'),
    (dict(k=1024), _is(('wide',), ACCEPTED, INVALID), 'k'),
    (dict(k=1025), INVALID, 'k'),
    (dict(stride=0), INVALID, 'shape'),
    (dict(stride=-2), INVALID, 'shape'),
    (dict(stride=7), ACCEPTED, None),
    (dict(P=0), INVALID, 'cells'),
    (dict(P=-1), INVALID, 'cells'),
    (dict(C=0), INVALID, 'cells'),
    (dict(C=16384), ACCEPTED, None),
    (dict(C=16385), INVALID, 'cells'),
    (dict(n_perm=-1, max_cell_rows=0), INVALID, 'cells'),
    (dict(n_perm=100), ACCEPTED, None),
    (dict(n_perm=101), INVALID, 'cells'),
    (dict(max_cell_rows=-1), INVALID, 'cells'),
    (dict(max_cell_rows=50), ACCEPTED, None),
    (dict(max_cell_rows=51), INVALID, 'cells'),
    (dict(max_probed_rows=-1), INVALID, 'cells'),
    (dict(max_probed_rows=0), ACCEPTED, None),
    (dict(max_probed_rows=10 ** 12), ACCEPTED, None),                        # (a bound the caller states: not held against n_perm)
    # B P = 2^32 with P small: refused where B * P is bounded, accepted where P alone is
    (dict(B=2 ** 20, P=4096), _is(BOUND_P, ACCEPTED, INVALID), 'cells'),
    (dict(B=INT32_MAX, P=1), ACCEPTED, None),
    (dict(B=0, P=2 ** 31), _is(BOUND_P, INVALID, OK), 'cells'),              # ... and the other way round where there are no queries
    (dict(centres=8, cell_of=8), ACCEPTED, None),
    (dict(centres=8, cell_of=8, metric=2), INVALID, 'centres'),
    (dict(centres=8, cell_of=8, metric=3), INVALID, 'centres'),
    (dict(centres=8, cell_of=8, metric=2, B=0), INVALID, 'centres'),         # (checked before "nothing to do")
    (dict(centres=8), INVALID, 'cell_of'),
    (dict(centres=8, B=0), INVALID, 'cell_of'),
    (dict(cell_of=8), ACCEPTED, None),                                       # (nobody reads it without centres)
    (dict(valid=8), ACCEPTED, None),                                         # what is optional: the live bitmap, what a stage hands back
    (dict(pn_out=8), ACCEPTED, None),
    (dict(qn_out=8), ACCEPTED, None),
    (dict(qx_out=8), ACCEPTED, None),
    (dict(scores=8), ACCEPTED, None),
    (dict(flags=1), ACCEPTED, None),
    (dict(ws_bytes=0), WORKSPACE, 'workspace'),
]
# nothing to do: OK with NULL everywhere, nothing is read.  (what varies, the code by job)
EARLY = [
    (dict(B=0), dict(search=OK, stage=OK, wide=OK)),
    (dict(B=0, N=0, n_perm=0, max_cell_rows=0), dict(search=OK, stage=OK, wide=OK)),
    (dict(n_perm=0, max_cell_rows=0), dict(search=INVALID, stage=OK, wide=INVALID)),  # a search over no rows still writes B answers
    (dict(N=0, n_perm=0, max_cell_rows=0), dict(search=INVALID, stage=OK, wide=INVALID)),
    (dict(B=0, metric=0), dict(search=INVALID, stage=INVALID, wide=INVALID)),         # (the checks come first)
    (dict(B=0, D=0), dict(search=INVALID, stage=INVALID, wide=INVALID)),
    (dict(B=0, C=0), dict(search=INVALID, stage=INVALID, wide=INVALID)),
    (dict(n_perm=0, max_cell_rows=0, stride=0), dict(search=INVALID, stage=INVALID, wide=INVALID)),
]


def test_every_entry_returns_its_code(capi):
    ran = [0] * len(CASES)
    for key in ENTRIES:
        for n, (kw, want, word) in enumerate(CASES):
            want = want(key) if callable(want) else want
            rc = _call(capi, key, **kw)
            if rc is None:
                continue  # (the entry has no such parameter)
            ran[n] += 1
            assert rc == want, (key, kw, rc, _err(capi))
            if word and rc == INVALID:
                assert word in _err(capi), (key, kw, _err(capi))
    assert all(ran), [CASES[n][0] for n, r in enumerate(ran) if not r]


def test_nothing_to_do_reads_no_pointer(capi):
    for key, (name, params) in ENTRIES.items():
        for kw, want in EARLY:
            kw = {p: v for p, v in kw.items() if p in params}
            rc = _raw(capi, key, **{p: None for p in POINTERS if p in params}, **kw)
            assert rc == want[key[0]], (key, kw, rc, _err(capi))


def test_each_required_pointer_in_turn(capi):
    for key, (name, params) in ENTRIES.items():
        required = [p for p in POINTERS if p in params]
        assert len(required) >= 7, key
        for p in required:
            assert _raw(capi, key, **{p: None}) == INVALID and 'null' in _err(capi), (key, p, _err(capi))
        # no rows in the cells: a stage has nothing to do; a search goes on, and needs neither the rows nor their norms nor the permutation
        empty = {p: v for p, v in dict(n_perm=0, max_cell_rows=0, x=None, perm=None, norms=None).items() if p in params}
        assert _call(capi, key, **empty) == (OK if key[0] == 'stage' else ACCEPTED), (key, _err(capi))
        if key[0] != 'stage':
            for p in ('cells', 'cell_rows', 'out_d', 'out_i'):
                assert _raw(capi, key, **empty, **{p: None}) == INVALID and 'null' in _err(capi), (key, p)


WS_ENTRIES = {'f32': 'annlite_ivf_flat_search_workspace_bytes', 'bf16x3': 'annlite_ivf_flat_search_split_workspace_bytes',
              'f16x2': 'annlite_ivf_flat_search_f16_workspace_bytes'}
# (B, P, C, D, k) -> the bytes of the f32, the bf16x3 and the f16x2 workspace
WS_BYTES = {
    (0, 4, 16, 8, 10): (512, 512, 512),
    (1, 1, 1, 1, 1): (18944, 27648, 19968),
    (4, 16, 16, 8, 10): (75776, 215040, 76800),                              # P = C
    (130, 8, 256, 100, 64): (2277376, 17551360, 2337280),                    # D no multiple of 16
    (7, 3, 5, 32768, 10): (119296, 84007936, 1037312),
    (1024, 16, 256, 128, 10): (17062400, 42424832, 17594880),
}
SPLIT = ('bf16x3', 'f16x2')
# (B, P, C, D, k) -> the code (the f32 entry takes no D)
WS_CODES = [
    ((4, 2, 16, 8, 10), OK),
    ((4, 2, 16, 8, 1), OK),
    ((4, 2, 16, 8, 64), OK),
    ((4, 2, 16, 8, 0), INVALID),
    ((4, 2, 16, 8, 65), INVALID),
    ((-1, 2, 16, 8, 10), INVALID),
    ((4, 0, 16, 8, 10), INVALID),
    ((4, 2, 0, 8, 10), INVALID),
    ((4, 2, 16385, 8, 10), OK),                                              # the size entries have never bounded C from above ...
    ((INT32_MAX + 1, 1, 16, 8, 10), OK),                                     # ... nor B
    ((4, 2, 16, 0, 10), _is(SPLIT, INVALID, OK)),
    ((4, 2, 16, 32769, 10), _is(SPLIT, INVALID, OK)),
]


def _ws_bytes(lib, f, B, P, C, D, k, out):
    args = (B, P, C, k) if f == 'f32' else (B, P, C, D, k)
    return getattr(lib, WS_ENTRIES[f])(*args, out)


def test_the_workspace_entries(capi):
    _capi, lib = capi
    n = ctypes.c_int64(0)
    assert len(WS_BYTES) >= 6
    for shape, want in WS_BYTES.items():
        got = []
        for f in FILTERS:
            assert _ws_bytes(lib, f, *shape, ctypes.byref(n)) == OK, (f, shape)
            got.append(n.value)
        assert tuple(got) == want, (shape, got)
    for shape, want in WS_CODES:
        for f in FILTERS:
            code = want(('ws', f)) if callable(want) else want
            assert _ws_bytes(lib, f, *shape, ctypes.byref(n)) == code, (f, shape)
    for f in FILTERS:
        assert _ws_bytes(lib, f, 4, 2, 16, 8, 10, None) == INVALID and 'bytes' in _err(capi)
