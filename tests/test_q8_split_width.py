"""The split step's first-phase width per launch (scan_q8.hip: q8_split_width, launch_q8_scan case 1650).  The kernel is one
template at HS = 10, 11, 12 (9 was swept too, lost at every slice length and is not compiled); a launch takes its width from
ANNLITE_Q8_SPLIT (forced) or from the rows one work item scans (ScanArgs::slice_rows against the threshold, ANNLITE_Q8_SPLIT_ROWS),
and says which one it took through annlite_debug_q8_split_width.  A narrower first phase only queues more rows for the unchanged full test: every width returns the
one-phase step's bits (ANNLITE_Q8_SPLIT=0) and the oracle's.

CPU: the bias-byte arithmetic at H = 9 and 10 (bias min(127 - T, 255 - 15 H); at 9 min(127 - T, 120), clamp 15 H - 128 = 7: the
arithmetic holds there, it was the measurement that dropped 9) and the ISA of the new instantiation -- no scratch, flat or s_load anywhere in the step loop, no v_readlane from the loop header to the vote's branch
nor in either block of the common trip, at most 128 VGPRs, and at most (6 H + 2) + 4 VALU instructions from the loop header to the
vote's branch (the look-ups' share plus the four of bookkeeping that test_q8_split_scalar_step.py allows).

GPU: the smallest shapes at which a width can go wrong -- fewer rows than one block, a ragged last block, one block past an
epoch's first 15, several epochs with a rebuild; one query, a ragged second tile, two full tiles; k = 1, 10, 16; deleted rows with a
whole block and the last row among them; a table with non-finite entries; bounds below the clamp; the selection rule."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import has_gpu
from test_isa_step_loop import _step_loop
from test_q8_split_bias import _window
from test_q8_split_scalar_step import _blocks, _loop
from test_q8_split_step import M, _bits, _structured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'annlite_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
gpu = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs an AMD GPU')]

WIDTHS = (10, 11, 12)  # every compiled first-phase width
NEW_WIDTHS = (10,)
ARITH_WIDTHS = (9, 10)
SYM = '_ZN7annlite18adc_scan_q8_kernelILi16ELi16ELb1ELi2ELi1ELb1ELi16ELb0ELi%dEEEvNS_8ScanArgsE'


# ------------------------------------------------------------------------------------------------- CPU: the byte arithmetic at H = 9, 10
def _bias(T, H):
    return np.minimum(127 - T, 255 - 15 * H)


@pytest.mark.parametrize('H', ARITH_WIDTHS)
def test_bias_bytes_exhaustively(H):
    T = np.arange(128)[:, None]
    S = np.arange(15 * H + 1)[None, :]
    b = _bias(T, H)
    assert np.all(b >= 0) and np.all(S + b <= 255)  # no byte carries at S <= 15 H
    clear = ((S + b) & 0x80) == 0
    assert np.array_equal(clear, S <= np.maximum(T, 15 * H - 128))  # bit 7 clear exactly when S <= max(T, 15 H - 128)
    assert 15 * H - 128 >= 0  # (a negative clamp would make bias = 255 - 15 H exceed 127: T = 0 would pass nothing)
    if H == 9:
        assert 15 * H - 128 == 7 and int(b.max()) == 120


@pytest.mark.parametrize('H', ARITH_WIDTHS)
def test_pad_slot_keeps_bit_7(H):
    """a pad slot's byte starts from 0x80 and its entries are clipped at 7: bit 7 stays, and the dword does not carry into the next slot"""
    S_pad = np.arange(7 * H + 1)
    assert np.all(0x80 + S_pad <= 255) and np.all((0x80 + S_pad) & 0x80)
    T = np.arange(128)[:, None, None]
    S = np.arange(15 * H + 1)[None, :, None]
    for lo in (True, False):
        word = ((0x80 + S_pad[None, None, :]) << (0 if lo else 8)) + ((S + _bias(T, H)) << (8 if lo else 0))
        nb = (word >> (8 if lo else 0)) & 0xff
        assert np.array_equal(nb, np.broadcast_to(S + _bias(T, H), nb.shape))
        assert np.all(((word >> (0 if lo else 8)) & 0x80) != 0) and np.all(word < 1 << 16)


# ------------------------------------------------------------------------------------------------- CPU: the ISA
@pytest.fixture(scope='module')
def asm_lines():
    if not os.path.exists(HIPCC):
        pytest.skip('hipcc not installed')
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, 'scan_q8.s')
        cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-mllvm',
               '-amdgpu-atomic-optimizer-strategy=None', '-S', '--cuda-device-only', 'scan_q8.hip', '-o', asm]
        subprocess.run(cmd, cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        return open(asm).read().splitlines()


@pytest.mark.parametrize('hs', NEW_WIDTHS)
def test_step_loop_of_the_new_widths(asm_lines, hs):
    sym = SYM % hs
    i0 = next(j for j, ln in enumerate(asm_lines) if ln.startswith(sym + ':'))
    i1 = next(j for j in range(i0, len(asm_lines)) if asm_lines[j].lstrip().startswith('.amdhsa_kernel ' + sym))
    body = asm_lines[i0:i1]
    loop = [ln.strip() for ln in _step_loop(body) if ln.startswith('\t') and not ln.lstrip().startswith((';', '.'))]
    assert sum(ln.startswith('ds_read_b128') for ln in loop) >= 2 * hs, (hs, 'the step loop was not found')
    # the whole loop, its rare parts (second phase, finish in place, epoch ends) included: no spill, no flat access, no scalar load
    bad = [ln for ln in loop if 'scratch_' in ln or re.match(r'flat_', ln) or ln.startswith(('s_load', 's_buffer_load'))]
    assert not bad, (hs, bad)
    assert not [ln for ln in body if re.search(r'\bflat_', ln) and not ln.lstrip().startswith(';')], hs
    # registers: the kernel's descriptor (16 waves per workgroup, one workgroup per CU: 128 VGPRs a lane)
    desc = asm_lines[i1:i1 + 80]
    vg = next(int(m.group(1)) for ln in desc for m in [re.search(r'\.amdhsa_next_free_vgpr\s+(\d+)', ln)] if m)
    print('HS = %d: %d VGPRs' % (hs, vg))
    assert vg <= 128, (hs, vg)
    # the common trip: two blocks back to back, no SGPR read back from a VGPR lane in either (as at HS = 11 and 12, the rare parts
    # reload a few spilled scalars)
    ins_all, _ = _loop(asm_lines, hs)
    blocks = _blocks(ins_all)
    assert len(blocks) == 2 and blocks[1][0] == blocks[0][2] + 1, (hs, blocks)
    for first, vote, end in blocks:
        trip = ins_all[first:end + 1]
        assert not [ln for ln in trip if 'scratch_' in ln or ln.startswith(('flat_', 'v_readlane', 'v_writelane', 's_load', 's_buffer_load'))], hs
        head = ins_all[first:vote + 1]
        assert sum(ln.startswith('v_') for ln in head) <= 6 * hs + 2 + 4, (hs, [ln for ln in head if ln.startswith('v_')])
        assert sum(ln.startswith('ds_read_b128') for ln in head) == 2 * hs, hs
    # the step-loop window: header to the vote's branch
    ins = _window(asm_lines, hs)
    assert not [ln for ln in ins if 'scratch_' in ln or ln.startswith(('flat_', 'v_readlane', 's_load', 's_buffer_load'))], hs
    n_valu = sum(ln.startswith('v_') for ln in ins)
    print('HS = %d: %d VALU instructions from the loop header to the vote (ceiling %d)' % (hs, n_valu, 6 * hs + 2 + 4))
    assert n_valu <= 6 * hs + 2 + 4, (hs, n_valu)
    assert sum(ln.startswith('ds_read_b128') for ln in ins) == 2 * hs, hs
    assert sum(ln.startswith('v_perm_b32') for ln in ins) == hs, hs


# ------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


N_ALL, B_ALL = 20_001, 64
N_CASES = [63, 65, 64 * 15 + 1, N_ALL]


@pytest.fixture(scope='module')
def data(ops, oracle):
    """one codec, one table, one batch and one set of float tables for every case below (the smaller tables are its first rows)"""
    cb, codes, q = _structured(ops, N_ALL, B_ALL, seed=41)
    cb_np, codes_np = cb.cpu().numpy(), ops.codes_to_numpy(codes)
    lut = oracle.batch_precompute_adc_table_c(q.cpu().numpy(), 8, 256, cb_np)
    return cb, codes, q, cb_np, codes_np, lut


def _run(ops, monkeypatch, env, q, cb, cs, k, vb=None):
    """one search on the byte-table plan with the switches in env; returns (distances, ids, split counters, entries pushed, width)"""
    import torch
    from annlite_amd import _capi
    from annlite_amd._capi import LUT_L2

    monkeypatch.setenv('ANNLITE_SCAN_VARIANT', '50')
    monkeypatch.setenv('ANNLITE_DEBUG_COUNTERS', '1')
    for name in ('ANNLITE_Q8_SPLIT', 'ANNLITE_Q8_SPLIT_ROWS'):
        if name in env:
            monkeypatch.setenv(name, env[name])
        else:
            monkeypatch.delenv(name, raising=False)
    _capi.knobs_reload()
    try:
        d, i = ops.pq_search_topk(LUT_L2, q, cb, cs, k, M, 256, codes_layout=1, valid_bits=vb)
        torch.cuda.synchronize()
        cnt = _capi.debug_split_counters()
        pushed = _capi.debug_counters()[1]
        width = _capi.debug_q8_split_width()
    finally:
        for name in ('ANNLITE_DEBUG_COUNTERS', 'ANNLITE_Q8_SPLIT', 'ANNLITE_Q8_SPLIT_ROWS'):
            monkeypatch.delenv(name, raising=False)
        _capi.knobs_reload()
    return d.cpu().numpy(), i.cpu().numpy(), cnt, pushed, width


def _holes(N):
    """a fifth of the rows invalid, the second 64-row block wholly (where the table has one), and the last row"""
    valid = np.ones(N, bool)
    valid[np.random.RandomState(N).choice(N, N // 5, replace=False)] = False
    if N >= 3 * 64:
        valid[64:128] = False
    valid[0] = True  # (at least one live row)
    valid[N - 1] = False
    return valid


def _all_widths(ops, oracle, monkeypatch, cb, codes, q, k, lut, codes_np, valid=None):
    """every width forced == the one-phase step == the oracle, bit for bit, and every launch is the kernel that was asked for"""
    monkeypatch.setenv('ANNLITE_SCAN_SLICES', '8')
    N = codes.shape[0]
    vb = None if valid is None else ops.to_dev(_bits(valid))
    cs = ops.codes_skew(codes)
    d0, i0, c0, _, w0 = _run(ops, monkeypatch, {'ANNLITE_Q8_SPLIT': '0'}, q, cb, cs, k, vb)
    assert w0 == 0 and c0 == [0, 0, 0, 0], (w0, c0)  # the byte-table plan was taken, with the one-phase step
    live = np.arange(N) if valid is None else np.nonzero(valid)[0]
    kk = min(k, len(live))
    with np.errstate(all='ignore'):
        rd, ri = oracle.adc_search_c(lut, codes_np[live], kk, threads=oracle.max_threads())
    assert np.array_equal(d0[:, :kk], rd, equal_nan=True) and np.array_equal(i0[:, :kk], live[ri])
    for hs in WIDTHS:
        d1, i1, c1, _, w1 = _run(ops, monkeypatch, {'ANNLITE_Q8_SPLIT': str(hs)}, q, cb, cs, k, vb)
        assert w1 == hs, (hs, w1)  # (not the previous launch's width, and not another plan's kernel)
        n_tiles = (q.shape[0] + 31) // 32
        assert c1[0] == len(live) * n_tiles, (hs, c1)  # every live row of every tile went through the first phase once
        assert np.array_equal(d1, d0, equal_nan=True) and np.array_equal(i1, i0), hs
        assert np.array_equal(d1[:, :kk], rd, equal_nan=True) and np.array_equal(i1[:, :kk], live[ri]), hs


@pytest.mark.parametrize('k', [1, 10, 16])
@pytest.mark.parametrize('B', [1, 33, 64])
@pytest.mark.parametrize('N', N_CASES)
def test_every_width_equals_the_one_phase_step_and_the_oracle(ops, oracle, monkeypatch, data, N, B, k):
    cb, codes, q, cb_np, codes_np, lut = data
    qq = q[:B].contiguous()
    _all_widths(ops, oracle, monkeypatch, cb, codes[:N], qq, k, lut[:B], codes_np[:N])
    _all_widths(ops, oracle, monkeypatch, cb, codes[:N], qq, k, lut[:B], codes_np[:N], valid=_holes(N))


def test_every_width_with_non_finite_tables(ops, oracle, monkeypatch):
    from test_round4_gpu import _nonfinite_inputs

    cb, x, q, kind = _nonfinite_inputs('huge_codewords_some', M, 8, N_ALL, 33, 256, seed=M * 31 + 9)
    codes = oracle.encode_c(x, np.where(np.isfinite(cb), cb, 0).astype(np.float32))
    with np.errstate(all='ignore'):
        lut = oracle.batch_precompute_adc_table_c(q, 8, 256, cb)
    assert not np.all(np.isfinite(lut))
    _all_widths(ops, oracle, monkeypatch, ops.to_dev(cb), ops.to_dev(codes), ops.to_dev(q), 10, lut, codes)


@pytest.mark.parametrize('hs', NEW_WIDTHS)
def test_bounds_below_the_clamp(ops, oracle, monkeypatch, data, hs):
    """16 queries, each the reconstruction of a table row r, and around each a tight cluster:
      among the first 4096 rows, the rows the first bound is taken from (ANNLITE_SEED_ROWS, ANNLITE_SEED_CONTIGUOUS): 12 exact copies
        of r -- the k-th distance is 0 from the first step on -- and 16 copies with ONE sub-space moved to the codeword at the median
        distance;
      rows [16448, N): 16 copies of r with j = 1 .. 8 sub-spaces (two rows each) moved to their FARTHEST codeword: table entries
        clipped at 15, S = 15 j.
    That the bounds are under the clamp 15 H - 128 = 22 is CHECKED, not assumed: of the 32 rows with j = 1 (S = 15) fewer than
    half pass the scanning waves' full test, so T < 15.  Then none of the 16 x 16 rows passes it, while a row survives the first
    phase when S_H <= max(T, 22), that is with at most ONE moved sub-space among its lane's first H: all of j = 1, 5/8 of j = 2,
    0.30 of j = 3, ... -- about 67 of the 256 (sd 4); with S_H <= T alone only those with NO moved sub-space there would,
    32 (6/16 + 1/8 + 1/28 + ...) = 17.5 (sd 3.5).  Survivors > rows passing the full test, by more than 17.5 + 5 sd = 35: the
    looser-below-the-clamp branch.  The rows are spread thinly (4 or 5 a block of 64): no step finishes in place, and every row
    passing the full test was a survivor first."""
    import torch

    cb, codes, _, cb_np, _, _ = data
    B, k = 16, 10
    for name, v in (('ANNLITE_SEED_CONTIGUOUS', '1'), ('ANNLITE_SEED_ROWS', '4096'), ('ANNLITE_SCAN_SLICES', '8')):
        monkeypatch.setenv(name, v)
    rs = np.random.RandomState(10)
    codes_np = ops.codes_to_numpy(codes).copy()
    src_row = 12288 + rs.choice(4096, B, replace=False)  # the rows r (left where they are: a 13th copy)
    src = codes_np[src_row].astype(np.int64)  # [B, M]
    planted = rs.choice(4096, 28 * B, replace=False).reshape(B, 28)
    seed, copies = planted[:, :16], planted[:, 16:]
    far = 16448 + rs.choice(N_ALL - 16448, 16 * B, replace=False).reshape(B, 8, 2)  # [b][j - 1][2]: j moved sub-spaces
    for b in range(B):
        codes_np[copies[b]] = src[b]
        order = []  # the codewords of sub-space m by their distance from r's (r's own last)
        for m in range(M):
            d2 = ((cb_np[m] - cb_np[m][src[b, m]]) ** 2).sum(axis=1)
            d2[src[b, m]] = np.inf
            order.append(np.argsort(d2))
            codes_np[seed[b, m]] = src[b]
            codes_np[seed[b, m], m] = order[m][127]
        for j in range(8):
            for r in range(2):
                codes_np[far[b, j, r]] = src[b]
                for m in rs.choice(M, j + 1, replace=False):
                    codes_np[far[b, j, r], m] = order[m][254]
    n_close = 16 * B + 12 * B + B  # the one-move copies, the exact copies and the rows r
    codes = ops.to_dev(codes_np)
    qq = torch.stack([cb[m][ops.to_dev(src[:, m])] for m in range(M)], dim=1).reshape(B, -1).contiguous()
    cs = ops.codes_skew(codes)
    d0, i0, _, _, w0 = _run(ops, monkeypatch, {'ANNLITE_Q8_SPLIT': '0'}, qq, cb, cs, k)
    d1, i1, c1, pushed, w1 = _run(ops, monkeypatch, {'ANNLITE_Q8_SPLIT': str(hs)}, qq, cb, cs, k)
    print('HS = %d: split counters %s, rows passing the full test %d, planted within one median move %d' % (hs, c1, pushed, n_close))
    assert (w0, w1) == (0, hs)
    assert np.array_equal(d1, d0) and np.array_equal(i1, i0)
    lut = oracle.batch_precompute_adc_table_c(qq.cpu().numpy(), 8, 256, cb_np)
    rd, ri = oracle.adc_search_c(lut, codes_np, k, threads=oracle.max_threads())
    assert np.array_equal(d1, rd) and np.array_equal(i1, ri)
    assert c1[3] == 0, c1  # (no step finished in place: every row that passed the full test went through the survivor ring)
    assert 0 < pushed < n_close + 2 * B // 2, (c1, pushed)  # fewer than half of the 2 B rows with S = 15 passed: T < 15 < 15 H - 128
    assert c1[1] - pushed > 35, (c1, pushed)


def test_selection_by_slice_length(ops, oracle, monkeypatch, data):
    from annlite_amd import _capi

    cb, codes, q, cb_np, codes_np, lut = data
    B, k = 33, 10
    qq = q[:B].contiguous()
    cs = ops.codes_skew(codes)
    monkeypatch.setenv('ANNLITE_SCAN_SLICES', '8')
    monkeypatch.setenv('ANNLITE_SCAN_VARIANT', '50')
    _capi.knobs_reload()
    ns = _capi.scan_plan(N_ALL, M, 256, 1, B, k).n_slices
    rows = ((N_ALL + ns - 1) // ns + 63) // 64 * 64  # the rows one work item scans (plan_slices)
    assert ns == 8 and rows == 2560
    cases = [  # (switches, the width the launch must report)
        ({}, 11),  # the compiled threshold is far above a 2560-row slice
        ({'ANNLITE_Q8_SPLIT_ROWS': '%d' % rows}, 10),  # a threshold at the slice length: reached
        ({'ANNLITE_Q8_SPLIT_ROWS': '%d' % (rows + 1)}, 11),  # ... one above it: not
        ({'ANNLITE_Q8_SPLIT_ROWS': '64'}, 10),
        ({'ANNLITE_Q8_SPLIT_ROWS': '1000000000'}, 11),
        ({'ANNLITE_Q8_SPLIT_ROWS': '0'}, 10),  # (a threshold of 0 rows is a threshold, not "unset")
        ({'ANNLITE_Q8_SPLIT_ROWS': '-5'}, 11),  # (negative: the compiled threshold)
        ({'ANNLITE_Q8_SPLIT_ROWS': '64', 'ANNLITE_Q8_SPLIT': '12'}, 12),  # a forced width wins over the rule
        ({'ANNLITE_Q8_SPLIT_ROWS': '64', 'ANNLITE_Q8_SPLIT': '11'}, 11),
        ({'ANNLITE_Q8_SPLIT_ROWS': '1000000000', 'ANNLITE_Q8_SPLIT': '10'}, 10),
        ({'ANNLITE_Q8_SPLIT_ROWS': '64', 'ANNLITE_Q8_SPLIT': '0'}, 0),
        ({'ANNLITE_Q8_SPLIT': '9'}, 11),  # (no such width is compiled: the rule decides)
        ({'ANNLITE_Q8_SPLIT': '9', 'ANNLITE_Q8_SPLIT_ROWS': '64'}, 10),
    ]
    rd, ri = oracle.adc_search_c(lut[:B], codes_np, k, threads=oracle.max_threads())
    for env, want in cases:
        d, i, c, _, w = _run(ops, monkeypatch, env, qq, cb, cs, k)
        assert w == want, (env, want, w)
        assert (c[0] > 0) == (want != 0), (env, c)
        assert np.array_equal(d, rd) and np.array_equal(i, ri), env


_CPU = {'test_bias_bytes_exhaustively', 'test_pad_slot_keeps_bit_7', 'test_step_loop_of_the_new_widths'}
for _name in [n for n in list(globals()) if n.startswith('test_') and n not in _CPU]:
    for _m in gpu:
        globals()[_name] = _m(globals()[_name])
