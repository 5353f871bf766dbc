"""What a PQ scan launch resolves to, pinned against the code it replaced.

``tests/golden/scan_launch_parent.json`` holds, per case, one record per scan launch as the commit before the host path was
restructured issued it on an MI355X: its ``scan_partial`` was patched (in scratch, never committed) to write the kernel family, id and
grid, every scalar kernel argument, every pointer argument as an offset from the workspace base (-1 NULL, -2 a buffer of the caller's),
the reset extent and the preparation launches with their seed rows just before each scan launch (and where the PREPARE half of the split
search returns), and the cases below were driven once through the public entries.  Here the same cases go to
``annlite_debug_scan_resolve`` -- pure host code, no GPU -- and every field must be equal.  The cases are the smallest that put each
threshold of the old function on both sides; ``_route`` says which launches an entry makes for a case (the record count checks it).
"""
import ctypes
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'scan_launch_parent.json')

HEAD = ['rc', 'stage', 'family', 'id', 'grid', 'skewed', 'fused_fill', 'fill_bytes', 'prep', 'mfma', 'S', 'S_prep', 'seed_extent', 'S_slice',
        'merged', 'plan_workspace_bytes', 'plan_n_slices', 'lds']
SCALARS = ['N', 'Ks', 'B', 'k', 'n_tiles', 'n_slices', 'n_items', 'slice_rows', 'jm1', 'row_base', 'sqrt_out', 'flush_mask', 'dbg_skip',
           'tl_private', 'cand_cap', 'q8_epoch0', 'q8_epoch_mul', 'q8_ring_limit', 'q8_import_mask', 'q8_target', 'q8_thw_mask',
           'q8_rebuild_8ths', 'guard_abort', 'guard_base', 'q8_early_merge', 'q8_merge_patience', 'q8_map_slices', 'q8_pos', 'q8_ilv_log']
POINTERS = ['codes', 'valid', 'lut', 'partial', 'smax', 'q16', 'qstep', 'qlo', 'qlom', 'gkey', 'gk2', 'gseed', 'tile_done', 'out_d', 'out_i',
            'out_packed', 'dbg', 'tile_rows', 'vmap', 'item_counter', 'cand', 'cand_count', 'guard', 'gate', 'host_stats', 'gseed0', 'btab']
FIELDS = HEAD + SCALARS + ['p_' + p for p in POINTERS]  # the order include/annlite_hip.h documents

SHARE, BUILD, TILES, GUARDED, GATED, STATE, CAND_SEED, PACKED, NO_OUT = 1, 2, 4, 8, 16, 32, 64, 128, 256
PREPARE, SCAN = 1, 2
KNOBS = ['SCAN_VARIANT', 'SCAN_SLICES', 'NO_FAST_CODE16', 'Q8_MAP', 'Q8_ILV', 'Q8_TARGET', 'Q8_REBUILD', 'Q8_TUNE', 'Q8_POS', 'SEED_ROWS',
         'SEED_CONTIGUOUS', 'NO_FUSED_SEED', 'NO_PREBUILT_TABLES', 'MFMA_SEED', 'GUARD_BASE', 'FLUSH_MASK', 'NO_EARLY_MERGE',
         'EARLY_MERGE_PATIENCE', 'NO_INKERNEL_MERGE', 'NO_FUSED_LUT', 'NO_CAND_SEED', 'DEBUG_COUNTERS', 'DEBUG_SKIP']


def _case(name, entry, N, B, k=10, M=16, Ks=256, cb=1, D=None, env=None, state=0, phase=0, seed_rows=0, V=0):
    """entry: the public function; state: 0 none, 1 the table's state has settled on byte tables, 2 on u16 tables; V: tile-mode slots"""
    return dict(name=name, entry=entry, N=N, B=B, k=k, M=M, Ks=Ks, cb=cb, D=D, env=env or {}, state=state, phase=phase, seed_rows=seed_rows, V=V)


def cases():
    out = []
    add = lambda *a, **kw: out.append(_case(*a, **kw))
    # ---- shapes and thresholds (tables handed over: annlite_adc_scan_topk) ----
    for N in (4095, 4096):  # a seed or none
        add('seed_N%d' % N, 'adc_scan_topk', N, 64)
    for N in (65535, 65536):  # k = 50: the byte-table kernel's 64-key lists need a table worth seeding
        add('lk64_N%d' % N, 'adc_scan_topk', N, 64, k=50)
    for N in (8 * 499968, 8 * 500032):  # 8 slices of 499 968 / 500 032 rows: how often the waves re-read the bounds
        add('thw_N%d' % N, 'adc_scan_topk', N, 1024)
    for N in (7999999, 8000000):  # M = 32: 8 slices and the slice-per-XCD map from 8M rows
        add('m32_N%d' % N, 'adc_scan_topk', N, 1024, M=32)
    for N in (200000, 500000, 2000000):  # N / 32 below 8192, between, above 32768: the seed rows' clamp
        add('sclamp_N%d' % N, 'adc_scan_topk', N, 64)
        add('sclamp_k50_N%d' % N, 'adc_scan_topk', N, 64, k=50)
    for B in (1, 2, 3):  # one tile that wants more than 128 slices
        add('onetile_B%d' % B, 'adc_scan_topk', 4000000, B)
    for B in (992, 1024, 1056):  # work items against the grid: the early merger
        add('items_B%d' % B, 'adc_scan_topk', 1000000, B)
    for N in (20000, 40000, 70000, 140000, 270000):  # 1, 2, 4, 8, 16 slices: the work items' rounding, the sibling group
        add('slices_N%d' % N, 'adc_scan_topk', N, 64)
        add('slices_k50_N%d' % N, 'adc_scan_topk', N, 64, k=50)
        add('slices_m8_N%d' % N, 'adc_scan_topk', N, 64, M=8)
        add('slices_cand_N%d' % N, 'adc_scan_candidates', N, 64)
    for k in (1, 16, 17, 50, 64):
        for M in (8, 16, 32):
            add('k%d_m%d' % (k, M), 'adc_scan_topk', 1000000, 1024, k=k, M=M)
        add('k%d_m16_small_batch' % k, 'adc_scan_topk', 1000000, 40, k=k)
        add('k%d_m16_cand' % k, 'adc_scan_candidates', 1000000, 256, k=k)
    for Ks in (256, 128):
        for k in (10, 50):
            add('m64_Ks%d_k%d' % (Ks, k), 'adc_scan_topk', 1000000, 256, k=k, M=64, Ks=Ks)
        add('m64_Ks%d_N8M' % Ks, 'adc_scan_topk', 4000000, 1024, M=64, Ks=Ks)
    for Ks in (512, 768):  # uint16 codes
        for k in (10, 50):
            add('u16_Ks%d_k%d' % (Ks, k), 'adc_scan_topk', 500000, 64, k=k, M=8, Ks=Ks, cb=2)
        add('u16_Ks%d_cand' % Ks, 'adc_scan_candidates', 500000, 64, M=8, Ks=Ks, cb=2)
    add('u16_m16_Ks512', 'adc_scan_topk', 500000, 64, M=16, Ks=512, cb=2)
    for B in (3, 300):  # the generic kernels: the fp32 table in LDS (one / two workgroups per CU), and not
        add('lds_B%d' % B, 'adc_scan_topk', 100000, B, M=24)
        add('lds_big_B%d' % B, 'adc_scan_topk', 100000, B, M=32, Ks=1024, cb=2)
        add('generic_B%d' % B, 'adc_scan_topk', 100000, B, M=48, Ks=1024, cb=4)
    add('lds_cand', 'adc_scan_candidates', 100000, 8, M=24)
    # ---- routes ----
    N, B = 1000000, 1024
    for e in ('adc_scan_topk', 'adc_scan_topk_packed', 'adc_scan_candidates'):
        add('route_' + e, e, N, B)
        add('route_' + e + '_skewed', e, N, B, env={'_layout': 1})
    for D in (128, 112, 512):  # 8-float sub-vectors; 7-float ones (no fusion); D > 256 (no one-launch preparation)
        add('route_pq_topk_D%d' % D, 'pq_search_topk', N, B, D=D)
        add('route_pq_topk_k50_D%d' % D, 'pq_search_topk', N, B, k=50, D=D)
        add('route_pq_cand_D%d' % D, 'pq_search_candidates', N, B, D=D)
        add('route_pq_tiles_D%d' % D, 'pq_search_tiles', N, 64, D=D, V=256)
    for M in (8, 32, 64):
        add('route_pq_topk_m%d' % M, 'pq_search_topk', N, B, M=M, D=128)
        add('route_pq_cand_m%d' % M, 'pq_search_candidates', N, B, M=M, D=128)
        add('route_pq_tiles_m%d' % M, 'pq_search_tiles', N, 64, M=M, D=128, V=256)
    add('route_pq_cand_small', 'pq_search_candidates', 4000, 64, D=128)
    add('route_pq_cand_no_cand_seed', 'pq_search_candidates', N, B, D=128, env={'NO_CAND_SEED': '1'})
    add('route_pq_cand_k50', 'pq_search_candidates', N, B, k=50, D=128)
    for sr in (0, 4096):
        for ph in (PREPARE, SCAN):
            add('route_split_%d_rows%d' % (ph, sr), 'pq_search_split', N, B, D=128, state=1, phase=ph, seed_rows=sr)
    for st in (1, 2):
        add('route_state%d_pq_topk' % st, 'pq_search_topk', N, B, D=128, state=st)
        add('route_state%d_pq_topk_k50' % st, 'pq_search_topk', N, B, k=50, D=128, state=st)
    add('route_state0_pq_topk', 'pq_search_topk', N, B, D=128, state=-1)  # a fresh state: guarded, with the statistics block
    # ---- switches, one each (M = 16, 1M rows, 1024 queries, k = 10) ----
    knobs = [{'Q8_MAP': '0'}, {'Q8_MAP': '1'}, {'Q8_ILV': '2'}, {'Q8_TARGET': '64'}, {'Q8_REBUILD': '6'}, {'Q8_TUNE': '3,2,192,0'},
             {'SEED_ROWS': '0'}, {'SEED_ROWS': '4096'}, {'SEED_CONTIGUOUS': '1'}, {'NO_FUSED_SEED': '1'}, {'NO_PREBUILT_TABLES': '1'},
             {'MFMA_SEED': '1'}, {'GUARD_BASE': '0'}, {'FLUSH_MASK': '31'}, {'NO_EARLY_MERGE': '1'}, {'EARLY_MERGE_PATIENCE': '100'},
             {'NO_INKERNEL_MERGE': '1'}, {'NO_FUSED_LUT': '1'}, {'SCAN_VARIANT': '31'}, {'SCAN_VARIANT': '50'}, {'SCAN_SLICES': '16'}]
    for env in knobs:
        (key, val), = env.items()
        add('knob_%s_%s' % (key, val.replace(',', '_')), 'pq_search_topk', N, B, D=128, env=env)
    add('knob_Q8_POS', 'pq_search_topk', N, B, k=50, D=128, env={'Q8_POS': '0.5,1.0,1.5,2.0'})
    add('knob_Q8_MAP_1_m64', 'adc_scan_topk', N, 256, M=64, env={'Q8_MAP': '0'})
    add('knob_SEED_ROWS_cand', 'pq_search_candidates', N, B, D=128, env={'SEED_ROWS': '4096', 'NO_CAND_SEED': '1'})
    add('knob_MFMA_SEED_state1', 'pq_search_topk', N, B, D=128, env={'MFMA_SEED': '1'}, state=1)
    add('knob_NO_FAST_CODE16', 'adc_scan_topk', 500000, 64, M=16, Ks=512, cb=2, env={'NO_FAST_CODE16': '1'})
    assert len({c['name'] for c in out}) == len(out)
    return out


def _route(c):
    """the scan launches a public entry makes for a case: [(variant, flags)] -- what search_policy and the entries decide"""
    M, Ks, cb, k, N, B, env, e = c['M'], c['Ks'], c['cb'], c['k'], c['N'], c['B'], c['env'], c['entry']
    both = (M in (8, 16, 32) and cb == 1 and Ks <= 256) or (M == 8 and cb == 2 and Ks <= 1024)
    fuse = c['D'] is not None and N > 0 and M != 64 and Ks <= 256 and (c['D'] // M) % 4 == 0 and 'NO_FUSED_LUT' not in env
    build = BUILD if fuse else 0
    if e in ('adc_scan_candidates', 'pq_search_candidates'):
        return [(-1, NO_OUT | build | (CAND_SEED if fuse and 'NO_CAND_SEED' not in env else 0))]
    if e == 'pq_search_tiles':
        return [(-1, SHARE | TILES | NO_OUT | build)]
    if e == 'pq_search_split':
        return [(50, SHARE | BUILD | STATE | PACKED)]
    out = PACKED if e == 'adc_scan_topk_packed' else 0
    plain = not both or (k > 16 and N < 65536) or 'SCAN_VARIANT' in env or 'NO_INKERNEL_MERGE' in env
    if plain:
        return [(-1, SHARE | build | (NO_OUT if 'NO_INKERNEL_MERGE' in env else out))]
    if c['state'] == 2:
        return [(31, SHARE | build | out)]
    if c['state'] == 1:
        return [(50, SHARE | build | out | STATE)]
    return [(50, SHARE | build | out | GUARDED | (STATE if c['state'] else 0)), (31, SHARE | out | GATED)]


def _environ(env):
    return {'ANNLITE_' + k: v for k, v in env.items() if not k.startswith('_')}


def _resolve(lib, c, variant, flags):
    out = (ctypes.c_int64 * len(FIELDS))()
    B, V = (c['V'], c['B']) if c['entry'] == 'pq_search_tiles' else (c['B'], 0)  # tile mode: B slots, V real queries
    lib.annlite_debug_scan_resolve(c['N'], c['M'], c['Ks'], c['cb'], c['env'].get('_layout', 0), B, c['k'], variant, flags, c['D'] or 0, V,
                                   c['phase'], c['seed_rows'], out, len(FIELDS))
    return dict(zip(FIELDS, (int(v) for v in out)))


@pytest.fixture(scope='module')
def lib():
    from annlite_amd import _capi

    L = _capi.lib()
    i64, i32 = ctypes.c_int64, ctypes.c_int
    L.annlite_debug_scan_resolve.argtypes = [i64, i64, i64, i32, i32, i64, i64, i32, i32, i64, i64, i32, i64, ctypes.POINTER(i64), i64]
    saved = {k: os.environ.pop('ANNLITE_' + k, None) for k in KNOBS}
    yield L
    for k, v in saved.items():
        os.environ.pop('ANNLITE_' + k, None)
        if v is not None:
            os.environ['ANNLITE_' + k] = v
    _capi.knobs_reload()


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    # stored small: "records" lists the launches in order as [case, base, {index in FIELDS: value}] -- the fields in which the launch
    # differs from launch number `base` of the list (-1: from nothing, every field is given)
    assert g['fields'] == FIELDS
    flat, out = [], {}
    for name, base, diff in g['records']:
        rec = list(flat[base]) if base >= 0 else [None] * len(FIELDS)
        for i, v in diff.items():
            rec[int(i)] = v
        flat.append(rec)
        out.setdefault(name, []).append(dict(zip(FIELDS, rec)))
    return out


def test_golden_covers_the_cases(golden):
    assert sorted(golden) == sorted(c['name'] for c in cases())
    fams = {r['family'] for recs in golden.values() for r in recs}
    assert fams == {0, 1, 2, 3}, fams  # byte tables, u16 tables, the generic kernel with and without the table in LDS
    assert any(r['stage'] == 2 for recs in golden.values() for r in recs)  # the PREPARE half


@pytest.mark.parametrize('c', cases(), ids=[c['name'] for c in cases()])
def test_resolve_matches_parent(lib, golden, c):
    from annlite_amd import _capi

    want, route = golden[c['name']], _route(c)
    assert len(want) == len(route), 'the parent made %d scan launches, the route says %d' % (len(want), len(route))
    env = _environ(c['env'])
    os.environ.update(env)
    _capi.knobs_reload()  # (the library parses its switches at load: tell it)
    try:
        got = [_resolve(lib, c, variant, flags) for variant, flags in route]
    finally:
        for k in env:
            del os.environ[k]
        _capi.knobs_reload()
    for g, w in zip(got, want):
        assert sorted(w) == sorted(FIELDS)
        diff = {f: (g[f], w[f]) for f in FIELDS if g[f] != w[f]}
        assert not diff, 'field: (resolved, parent) %r' % diff
