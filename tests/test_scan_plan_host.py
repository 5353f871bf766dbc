"""The scan plan of the PQ host path, pinned: ``annlite_scan_plan_query``, ``annlite_scan_plan_tiles``,
``annlite_pq_search_workspace_bytes`` and ``annlite_pq_search_tiles_workspace_bytes`` over a grid of shapes, k, batch sizes, table
sizes and ``ANNLITE_SCAN_VARIANT`` values: all eight plan fields and the return code of every call, exactly.  The golden
(``tests/golden/scan_plan_parent.json``) was recorded from a build of the commit before the host path was restructured
(``python tests/test_scan_plan_host.py`` writes it).  To stay small it holds, per (setting, shape, k), the first 64 bits of the
SHA-256 of the 42 (B, N) cases' values in their canonical form below -- equal digests are equal values; a block that differs is
printed in full -- and the two single-case settings in plain.  The plan functions make no device call, so this runs without a GPU, where the library takes 256
compute units -- the MI355X's own count.
"""
import ctypes
import hashlib
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scan_plan_parent.json')

SHAPES = [(8, 256, 1), (16, 256, 1), (32, 256, 1), (64, 256, 1), (64, 128, 1), (8, 512, 2), (8, 768, 2), (8, 1025, 2), (16, 512, 2),
          (24, 256, 1), (48, 1024, 4)]
KS = [1, 16, 17, 64, 65]
BS = [0, 1, 3, 32, 33, 1024]
NS = [0, 63, 4096, 65536, 1000000, 8000000, 2 ** 32 - 1]
VARIANTS = [None, 30, 31, 32, 50]
# the two further settings, one case each ((M, Ks, code bytes), k, B, N): a batch whose plan the switch changes; uint16 codes that
# leave the fast plan
EXTRA = [('slices16', {'ANNLITE_SCAN_SLICES': '16'}, ((16, 256, 1), 10, 1024, 1000000)),
         ('no_fast_code16', {'ANNLITE_NO_FAST_CODE16': '1'}, ((8, 512, 2), 10, 32, 65536))]
PLAN_FIELDS = ('fast', 'qi', 'qt', 'waves', 'n_slices', 'max_k', 'lut_floats', 'workspace_bytes')


def _settings():
    return [('variant_%s' % ('unset' if v is None else v), {} if v is None else {'ANNLITE_SCAN_VARIANT': str(v)}) for v in VARIANTS]


def _case(lib, ScanPlan, shape, k, B, N):
    """[rc, 8 fields] of both plans, [rc, bytes] of both workspace entries; a refused call reports its return code alone"""
    M, Ks, cb = shape
    row = []
    for fn in (lib.annlite_scan_plan_query, lib.annlite_scan_plan_tiles):
        p = ScanPlan()
        rc = fn(N, M, Ks, cb, B, k, ctypes.byref(p))
        row.append([rc] + ([int(getattr(p, f)) for f in PLAN_FIELDS] if rc == 0 else []))
    for fn in (lib.annlite_pq_search_workspace_bytes, lib.annlite_pq_search_tiles_workspace_bytes):
        b = ctypes.c_int64(-1)
        rc = fn(N, M, Ks, cb, B, k, ctypes.byref(b))
        row.append([rc] + ([int(b.value)] if rc == 0 else []))
    return row


def _under(env, fn):
    """fn(lib, ScanPlan) with the switches of ``env`` and no others of the plan's set"""
    from annlite_amd import _capi

    lib = _capi.lib()
    saved = {v: os.environ.get(v) for v in ('ANNLITE_SCAN_VARIANT', 'ANNLITE_SCAN_SLICES', 'ANNLITE_NO_FAST_CODE16')}
    for v in saved:
        os.environ.pop(v, None)
    os.environ.update(env)
    _capi.knobs_reload()  # (the library parses its switches at load: tell it)
    try:
        return fn(lib, _capi.ScanPlan)
    finally:
        for v, old in saved.items():
            os.environ.pop(v, None)
            if old is not None:
                os.environ[v] = old
        _capi.knobs_reload()


def _blocks(lib, ScanPlan):
    """{'M,Ks,bytes,k': rows of the 42 (B, N) cases}"""
    return {'%d,%d,%d,k%d' % (s + (k,)): [_case(lib, ScanPlan, s, k, B, N) for B in BS for N in NS] for s in SHAPES for k in KS}


def _digest(rows):
    return hashlib.sha256(json.dumps(rows, separators=(',', ':')).encode()).hexdigest()[:16]


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize('name,env', _settings(), ids=[s[0] for s in _settings()])
def test_plan_matches_parent(golden, name, env):
    got, want = _under(env, _blocks), golden[name]
    assert sorted(got) == sorted(want)
    bad = [b for b in got if _digest(got[b]) != want[b]]
    assert not bad, '%d of %d blocks differ from the parent; first: %s, rows over B in %r x N in %r: %r' % (
        len(bad), len(got), bad[0], BS, NS, got[bad[0]])


@pytest.mark.parametrize('name,env,case', EXTRA, ids=[e[0] for e in EXTRA])
def test_plan_switch_matches_parent(golden, name, env, case):
    assert _under(env, lambda lib, P: _case(lib, P, *case)) == golden[name]


def test_refusals_and_both_plans():
    """k = 65 and N = 2^32 - 1 are refused, everything else is planned; fast and generic plans both occur"""
    blocks = _under({}, _blocks)
    fast = set()
    for name, rows in blocks.items():
        for (B, N), row in zip(((B, N) for B in BS for N in NS), rows):
            refused = name.endswith('k65') or N == 2 ** 32 - 1
            assert all((r[0] != 0) == refused for r in row), (name, B, N, row)
            if not refused:
                fast.add(row[0][1])
    assert fast == {0, 1}


if __name__ == '__main__':
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = {name: {b: _digest(rows) for b, rows in _under(env, _blocks).items()} for name, env in _settings()}
    out.update({name: _under(env, lambda lib, P: _case(lib, P, *case)) for name, env, case in EXTRA})
    J = lambda x: json.dumps(x, separators=(',', ':'))
    lines = ['%s:{\n%s}' % (J(name), ',\n'.join(','.join('%s:%s' % (J(b), J(d)) for b, d in list(v.items())[i:i + len(KS)])
                                                for i in range(0, len(v), len(KS)))) if isinstance(v, dict) else '%s:%s' % (J(name), J(v))
             for name, v in out.items()]  # (one line per shape)
    with open(GOLDEN, 'w') as f:
        f.write('{' + ',\n'.join(lines) + '}\n')
    print('wrote', GOLDEN, os.path.getsize(GOLDEN), 'bytes')
