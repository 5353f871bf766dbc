"""The split step's first phase with BIAS words (scan_q8.hip, split_first / split_pass1, q8_st_bound): a slot with bound byte
0x80 | T keeps bias = min(127 - T, 255 - 15 H); the first phase's byte sums (H sub-spaces, entries <= 15: S_H <= 15 H) start from
the bias bytes, never carry, and bit 7 of a byte is clear exactly when S_H <= max(T, 15 H - 128) -- the round-8 decision S_H <= T
bit for bit down to T = 15 H - 128, looser below, never stricter.  A pad slot (byte 0x7f) keeps bias 0x80 and never passes.  The rare parts (finish in place, second phase) take the bias
out and test full sums against the filter words as before.

CPU: the byte arithmetic, exhaustively, and the ISA of the hot window.  VALU instructions from the loop header to the vote's
branch, counted by this file's `_window` on the parent commit and on this one:

    HS = 11:  parent 99, with bias words 77        HS = 12:  parent 100, with bias words 78

GPU: the places where the bias matters -- bounds below the clamp, T = 127, deleted rows, steps that finish in place (the bias is
taken out of the sums), non-finite tables, rebuilds and epoch ends, a full and a one-query tile -- against the one-phase step
(ANNLITE_Q8_SPLIT=0) and the oracle, distances and ids bit for bit."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import has_gpu
from test_isa_step_loop import _step_loop
from test_q8_split_step import M, _bits, _search, _structured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'annlite_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
gpu = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs an AMD GPU')]

HS_ALL = (10, 11, 12)
PARENT_VALU = {11: 99, 12: 100}
NEW_VALU = {11: 77, 12: 78}
DEPTH = 8  # ANNLITE_Q8_DEPTH: look-ups of the next block in flight when a step votes


def _bias(T, H):
    return np.minimum(127 - T, 255 - 15 * H)


# ------------------------------------------------------------------------------------------------- CPU: the byte arithmetic
@pytest.mark.parametrize('H', HS_ALL)
def test_bias_bytes_exhaustively(H):
    T = np.arange(128)[:, None]
    S = np.arange(15 * H + 1)[None, :]
    b = _bias(T, H)
    assert np.all(b >= 0) and np.all(S + b <= 255)  # a byte never carries
    clear = ((S + b) & 0x80) == 0
    exact = np.broadcast_to(T >= 15 * H - 128, clear.shape)
    assert np.array_equal(clear[exact], (S <= T)[exact])  # the round-8 decision, bit for bit
    assert np.all(clear[(S <= T) & ~exact])  # below the clamp: looser, never stricter
    assert np.array_equal(clear, S <= np.maximum(T, 15 * H - 128))


@pytest.mark.parametrize('H', HS_ALL)
def test_pad_slot_byte_keeps_bit_7_and_never_carries(H):
    """a pad slot (bound byte 0x7f, no flag bit) keeps bias 0x80; its table is all zero, and whatever a build leaves there is clipped
    at QOPEN = 7: for every such sum the byte keeps bit 7 (never passes, as with the filter words) and the dword does not carry into
    the neighbouring slot, whose answer stays its own"""
    S_pad = np.arange(7 * H + 1)
    assert np.all(0x80 + S_pad <= 255) and np.all((0x80 + S_pad) & 0x80)
    T = np.arange(128)[:, None, None]
    S = np.arange(15 * H + 1)[None, :, None]
    for lo in (True, False):  # the pad slot below / above its neighbour in the dword
        word = ((0x80 + S_pad[None, None, :]) << (0 if lo else 8)) + ((S + _bias(T, H)) << (8 if lo else 0))
        nb = (word >> (8 if lo else 0)) & 0xff
        assert np.array_equal(nb, np.broadcast_to(S + _bias(T, H), nb.shape))
        assert np.all(((word >> (0 if lo else 8)) & 0x80) != 0) and np.all(word < 1 << 16)
    assert (~np.uint8(0x80)) == 0x7f  # (its complement is the pad slot's filter byte again)


@pytest.mark.parametrize('H', HS_ALL)
def test_bias_bytes_packed_four_to_a_dword(H):
    rs = np.random.RandomState(H)
    n = 100_000
    T = rs.randint(0, 128, size=(n, 4))
    low = rs.rand(n, 4) < 0.3
    T[low] = rs.randint(0, 15 * H - 127, size=int(low.sum()))  # (plenty at and below the clamp)
    ent = rs.randint(0, 16, size=(n, H, 4))
    ent[rs.rand(n, H, 4) < 0.2] = 15  # (sums up to 15 H)
    S = ent.sum(axis=1)
    b = _bias(T, H)
    pack = lambda a: (a.astype(np.uint32) << (8 * np.arange(4, dtype=np.uint32))).sum(axis=1, dtype=np.uint64)
    acc = pack(b)
    for h in range(H):
        acc = acc + pack(ent[:, h])
    assert np.all(acc < 2 ** 32)
    acc = acc.astype(np.uint32)
    for i in range(4):
        by = (acc >> np.uint32(8 * i)) & np.uint32(0xff)
        assert np.array_equal(by, (S[:, i] + b[:, i]).astype(np.uint32))  # nothing crosses a byte
        assert np.array_equal((by & 0x80) == 0, S[:, i] <= np.maximum(T[:, i], 15 * H - 128))
    # the test itself: any byte of the dword with bit 7 clear
    assert np.array_equal((~acc & np.uint32(0x80808080)) != 0, np.any(S <= np.maximum(T, 15 * H - 128), axis=1))
    # taking the bias out again borrows nothing
    assert np.array_equal(acc - pack(b).astype(np.uint32), pack(S).astype(np.uint32))


@pytest.mark.parametrize('H', HS_ALL)
def test_complement_of_a_bias_byte_is_a_filter_byte(H):
    T = np.arange(128)
    b = _bias(T, H)
    assert np.array_equal((~b.astype(np.uint8)), (0x80 | (127 - b)).astype(np.uint8))
    assert np.all(127 - b >= T)  # (looser only where the clamp bit)
    assert np.array_equal((127 - b)[T >= 15 * H - 128], T[T >= 15 * H - 128])


# ------------------------------------------------------------------------------------------------- CPU: the ISA
def _window(lines, hs):
    """instructions from the step loop's header to the vote's branch"""
    sym = '_ZN7annlite18adc_scan_q8_kernelILi16ELi16ELb1ELi2ELi1ELb1ELi16ELb0ELi%dEEEvNS_8ScanArgsE' % hs
    i0 = next(j for j, ln in enumerate(lines) if ln.startswith(sym + ':'))
    i1 = next(j for j in range(i0, len(lines)) if lines[j].lstrip().startswith('.amdhsa_kernel ' + sym))
    ins = [ln.strip() for ln in _step_loop(lines[i0:i1]) if ln.startswith('\t') and not ln.lstrip().startswith((';', '.'))]
    pop = next(j for j, ln in enumerate(ins) if ln.startswith('s_bcnt1_i32_b64'))
    branch = next(j for j in range(pop, len(ins)) if ins[j].startswith('s_cbranch'))
    return ins[:branch]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_hot_window_has_the_one_bit_test():
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, 'scan_q8.s')
        cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-mllvm',
               '-amdgpu-atomic-optimizer-strategy=None', '-S', '--cuda-device-only', 'scan_q8.hip', '-o', asm]
        subprocess.run(cmd, cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        lines = open(asm).read().splitlines()
    for hs in (11, 12):  # (the default and ANNLITE_Q8_SPLIT=12)
        ins = _window(lines, hs)
        assert not [ln for ln in ins if ln.startswith('v_sub_u32')], hs
        assert not [ln for ln in ins if '0x7f7f7f7f' in ln], hs
        n_valu = sum(ln.startswith('v_') for ln in ins)
        print('HS = %d: %d VALU instructions from the loop header to the vote (parent: %d)' % (hs, n_valu, PARENT_VALU[hs]))
        assert n_valu <= PARENT_VALU[hs] - 20, (hs, n_valu)
        assert n_valu <= NEW_VALU[hs] + 3, (hs, n_valu)
        # the test: an AND tree over the 8 accumulator dwords closed against 0x80808080, and the compare
        n_test = sum(ln.startswith(('v_bitop3_b32', 'v_or3_b32', 'v_and_or_b32')) for ln in ins)
        assert n_test <= 5, (hs, n_test)
        reads = [j for j, ln in enumerate(ins) if ln.startswith('ds_read_b128')]
        assert len(reads) >= 2 * hs, (hs, reads)
        drains = [ln for ln in ins[reads[-DEPTH]:] if re.match(r's_waitcnt\s+.*lgkmcnt\(0\)', ln)]
        assert not drains, (hs, 'the LDS queue drains between the next block\'s first look-ups and the vote', drains)


# ------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


N_ALL, B_ALL = 70_001, 33  # (B = 33: one full tile, one tile with 31 pad slots)


@pytest.fixture(scope='module')
def data(ops):
    """one codec, one table and one batch for every case below (the smaller table is its first 20 000 rows)"""
    cb, codes, q = _structured(ops, N_ALL, B_ALL, seed=29)
    return cb, codes, q, cb.cpu().numpy(), ops.codes_to_numpy(codes)


def _check(ops, oracle, monkeypatch, cb, codes, q, k, valid=None, cb_np=None, codes_np=None):
    """split step == one-phase step == oracle, all queries, bit for bit; returns the split counters"""
    monkeypatch.setenv('ANNLITE_SCAN_SLICES', '8')
    N = codes.shape[0]
    vb = None if valid is None else ops.to_dev(_bits(valid))
    cs = ops.codes_skew(codes)
    d1, i1, c1 = _search(ops, monkeypatch, True, q, cb, cs, k, vb)
    d0, i0, c0 = _search(ops, monkeypatch, False, q, cb, cs, k, vb)
    print('split counters (rows, survivors, second-phase wave-steps, finished in place):', c1)
    assert c1[0] > 0 and c0 == [0, 0, 0, 0], (c1, c0)
    assert np.array_equal(d1, d0, equal_nan=True) and np.array_equal(i1, i0)
    cb_np = cb.cpu().numpy() if cb_np is None else cb_np
    codes_np = ops.codes_to_numpy(codes) if codes_np is None else codes_np
    live = np.arange(N) if valid is None else np.nonzero(valid)[0]
    kk = min(k, len(live))
    with np.errstate(all='ignore'):
        lut = oracle.batch_precompute_adc_table_c(q.cpu().numpy(), 8, 256, cb_np)
        rd, ri = oracle.adc_search_c(lut, codes_np[live], kk, threads=oracle.max_threads())
    assert np.array_equal(d1[:, :kk], rd, equal_nan=True) and np.array_equal(i1[:, :kk], live[ri])
    return c1


@pytest.mark.parametrize('k', [1, 10, 16])
@pytest.mark.parametrize('N', [20_000, N_ALL])
def test_default_sizes(ops, oracle, monkeypatch, data, N, k):
    cb, codes, q, cb_np, codes_np = data
    _check(ops, oracle, monkeypatch, cb, codes[:N], q, k, cb_np=cb_np, codes_np=codes_np[:N])


def _copies(ops, monkeypatch, data, N, seed):
    """the first N rows with 12 copies of B_ALL of them among the first 8192, the queries their reconstructions, and the first bound
    taken from those 8192 rows"""
    import torch

    cb, codes = data[0], data[1]
    monkeypatch.setenv('ANNLITE_SEED_CONTIGUOUS', '1')
    rs = np.random.RandomState(seed)
    codes = codes[:N].clone()
    pos = rs.choice(8192, 12 * B_ALL, replace=False).reshape(B_ALL, 12)
    pos_d = ops.to_dev(pos.astype(np.int64))
    for c in range(1, 12):
        codes[pos_d[:, c]] = codes[pos_d[:, 0]]
    src = codes[pos_d[:, 0]].long()  # [B, M]
    qq = torch.stack([cb[m][src[:, m]] for m in range(M)], dim=1).reshape(B_ALL, -1).contiguous()
    return codes, qq


@pytest.mark.parametrize('k', [1, 10])
@pytest.mark.parametrize('N', [20_000, N_ALL])
def test_bounds_below_the_clamp(ops, oracle, monkeypatch, data, N, k):
    """every query is the reconstruction of a table row that the table holds 12 times, all of them among the rows the first bound is
    taken from (the table's first 8192: ANNLITE_SEED_CONTIGUOUS): the k-th distance is 0 and T near 0 from the first step on, far below
    15 H - 128 -- the first phase runs on the clamp.  (Left to the scan to find, the copies of a table this small are found when its
    few steps per wave are over.)"""
    cb, _, _, cb_np, _ = data
    codes, qq = _copies(ops, monkeypatch, data, N, seed=N + k)
    c1 = _check(ops, oracle, monkeypatch, cb, codes, qq, k, cb_np=cb_np)
    assert c1[1] > 0 and c1[2] > 0, c1  # survivors and second-phase wave-steps: the loosened branch ran


@pytest.mark.parametrize('B', [1, B_ALL])
def test_pad_slots_never_pass(ops, oracle, monkeypatch, data, B):
    """a ragged tile (31 pad slots beside one query, alone or behind a full tile) filters like a full one: a pad slot's byte starts
    from 0x80 and keeps bit 7, so the rows are dropped on the real slots' bounds (tight here: the queries of
    test_bounds_below_the_clamp) and next to no step finishes in place.  (A pad slot that passed would send EVERY step there.)"""
    cb, _, _, cb_np, _ = data
    codes, qq = _copies(ops, monkeypatch, data, N_ALL, seed=B)
    c1 = _check(ops, oracle, monkeypatch, cb, codes, qq[:B].contiguous(), 1, cb_np=cb_np)
    assert c1[1] > 0 and c1[3] * 10 < c1[0] // 64, c1


@pytest.mark.parametrize('k', [10, 16])
def test_fewer_than_k_valid_rows(ops, oracle, monkeypatch, data, k):
    """T = 127 (bias 0) throughout: the lists never fill"""
    cb, codes, q, cb_np, codes_np = data
    valid = np.zeros(N_ALL, bool)
    valid[[5, 64 * 300 + 1, 64 * 300 + 2, 40_000, N_ALL - 1]] = True
    _check(ops, oracle, monkeypatch, cb, codes, q, k, valid=valid, cb_np=cb_np, codes_np=codes_np)


@pytest.mark.parametrize('N', [20_000, N_ALL])
def test_deleted_rows(ops, oracle, monkeypatch, data, N):
    cb, codes, q, cb_np, codes_np = data
    valid = np.ones(N, bool)
    valid[np.random.RandomState(N).choice(N, N // 5, replace=False)] = False
    valid[-40:] = False  # (the last block: partly deleted, partly live)
    valid[-7] = True
    _check(ops, oracle, monkeypatch, cb, codes[:N], q, 10, valid=valid, cb_np=cb_np, codes_np=codes_np[:N])


def test_uniform_codes_finish_in_place(ops, oracle, monkeypatch):
    """independent random codes: most steps finish in place -- the bias is taken out of the first-phase sums"""
    rs = np.random.RandomState(17)
    cb = rs.randn(M, 256, 8).astype(np.float32)
    codes = rs.randint(0, 256, size=(N_ALL, M)).astype(np.uint8)
    q = rs.randn(B_ALL, M * 8).astype(np.float32)
    c1 = _check(ops, oracle, monkeypatch, ops.to_dev(cb), ops.to_dev(codes), ops.to_dev(q), 10, cb_np=cb, codes_np=codes)
    assert c1[3] > 0, c1


@pytest.mark.parametrize('case', ['inf_query', 'nan_query', 'huge_codewords_some'])
def test_non_finite_tables(ops, oracle, monkeypatch, case):
    from test_round4_gpu import _nonfinite_inputs

    cb, x, q, kind = _nonfinite_inputs(case, M, 8, 20_000, B_ALL, 256, seed=M * 31 + 10)
    codes = oracle.encode_c(x, np.where(np.isfinite(cb), cb, 0).astype(np.float32) if case.startswith('huge') else cb)
    _check(ops, oracle, monkeypatch, ops.to_dev(cb), ops.to_dev(codes), ops.to_dev(q), 10, cb_np=cb, codes_np=codes)


@pytest.mark.parametrize('tune', ['1,2,192,0', '1,2,192,3'])
def test_forced_rebuilds_and_epoch_ends(ops, oracle, monkeypatch, data, tune):
    """the closest epoch ends the switches allow (ANNLITE_Q8_TUNE=1,2,...: after steps 1, 3, 7, 15, ... -- the multiplier is at least
    2, so an end after every other step cannot be forced) and a rebuild as soon as a bound moves: with about 9 steps per wave that is
    three epoch ends per work item, at each of which both arrays of bounds are written again and the bias words picked up"""
    cb, codes, q, cb_np, codes_np = data
    monkeypatch.setenv('ANNLITE_Q8_TUNE', tune)
    monkeypatch.setenv('ANNLITE_Q8_TARGET', '64')
    monkeypatch.setenv('ANNLITE_Q8_REBUILD', '7')
    _check(ops, oracle, monkeypatch, cb, codes, q, 10, cb_np=cb_np, codes_np=codes_np)


@pytest.mark.parametrize('B', [32, 1])
def test_full_tile_and_one_query(ops, oracle, monkeypatch, data, B):
    cb, codes, q, cb_np, codes_np = data
    _check(ops, oracle, monkeypatch, cb, codes, q[:B].contiguous(), 10, cb_np=cb_np, codes_np=codes_np)


_CPU = {'test_pad_slot_byte_keeps_bit_7_and_never_carries', 'test_bias_bytes_exhaustively', 'test_bias_bytes_packed_four_to_a_dword', 'test_complement_of_a_bias_byte_is_a_filter_byte',
        'test_hot_window_has_the_one_bit_test'}
for _name in [n for n in list(globals()) if n.startswith('test_') and n not in _CPU]:
    for _m in gpu:
        globals()[_name] = _m(globals()[_name])
