"""The split step's first-phase look-ups run across the step boundary (scan_q8.hip, split_first / split_prefix): a step issues the
next block's first look-ups into the landing ring behind its own last ones, so that its drain, pass test and vote run with
look-ups in flight; the rare parts (finish in place, second phase) and every epoch entry issue that prefix again.  The CPU test
pins the order in the ISA; the GPU tests run the places where the prefix is dropped and issued again -- epoch ends after every
other step, ragged and tiny slices, a partly deleted last block, deleted rows, uniform codes (most steps finish in place), forced
rebuilds, non-finite tables -- against the one-phase step (ANNLITE_Q8_SPLIT=0) and the oracle."""
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

DEPTH = 8  # ANNLITE_Q8_DEPTH: look-ups of the next block in flight when a step votes
VALU_CEILING = 104  # VALU instructions from the loop header to the vote's branch (99 / 100 at HS = 11 / 12 when the prefix went in)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_next_block_lookups_in_flight_across_the_vote():
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, 'scan_q8.s')
        cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-mllvm',
               '-amdgpu-atomic-optimizer-strategy=None', '-S', '--cuda-device-only', 'scan_q8.hip', '-o', asm]
        subprocess.run(cmd, cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        lines = open(asm).read().splitlines()
    for hs in (11, 12):  # (the default and ANNLITE_Q8_SPLIT=12)
        _check_step_loop(lines, hs)


def _check_step_loop(lines, hs):
    sym = '_ZN7annlite18adc_scan_q8_kernelILi16ELi16ELb1ELi2ELi1ELb1ELi16ELb0ELi%dEEEvNS_8ScanArgsE' % hs
    i0 = next(j for j, ln in enumerate(lines) if ln.startswith(sym + ':'))
    i1 = next(j for j in range(i0, len(lines)) if lines[j].lstrip().startswith('.amdhsa_kernel ' + sym))
    window = _step_loop(lines[i0:i1])
    ins = [ln.strip() for ln in window if ln.startswith('\t') and not ln.lstrip().startswith((';', '.'))]
    # the vote: the popcount of the ballot of the pass test, then the branch on it
    pop = next(j for j, ln in enumerate(ins) if ln.startswith('s_bcnt1_i32_b64'))
    branch = next(j for j in range(pop, len(ins)) if ins[j].startswith('s_cbranch'))
    reads = [j for j in range(branch) if ins[j].startswith('ds_read_b128')]
    assert len(reads) >= 2 * hs, (hs, reads)  # (the step's own look-ups and the next block's first ones)
    tail = ins[reads[-DEPTH]:branch]
    drains = [ln for ln in tail if re.match(r's_waitcnt\s+.*lgkmcnt\(0\)', ln)]
    assert not drains, (hs, 'the LDS queue drains between the next block\'s first look-ups and the vote', drains)
    n_valu = sum(ln.startswith('v_') for ln in ins[:branch])
    assert n_valu <= VALU_CEILING, (hs, n_valu)


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _check(ops, oracle, monkeypatch, N, B, k, seed, deleted):
    cb, codes, q = _structured(ops, N, B, seed=seed)
    valid = np.ones(N, bool)
    vb = None
    if deleted:
        rs = np.random.RandomState(seed)
        valid[rs.choice(N, N // 5, replace=False)] = False
        valid[-40:] = False  # (the last block: partly deleted, partly live)
        valid[-7] = True
        vb = ops.to_dev(_bits(valid))
    cs = ops.codes_skew(codes)
    d1, i1, c1 = _search(ops, monkeypatch, True, q, cb, cs, k, vb)
    d0, i0, _ = _search(ops, monkeypatch, False, q, cb, cs, k, vb)
    assert c1[0] > 0, c1
    assert np.array_equal(d1, d0) and np.array_equal(i1, i0)
    nq = min(B, 8)
    lut = oracle.batch_precompute_adc_table_c(q[:nq].cpu().numpy(), 8, 256, cb.cpu().numpy())
    live = np.nonzero(valid)[0]
    rd, ri = oracle.adc_search_c(lut, ops.codes_to_numpy(codes)[live], k, threads=oracle.max_threads())
    assert np.array_equal(d1[:nq], rd) and np.array_equal(i1[:nq], live[ri])
    return c1


@pytest.mark.parametrize('N', [64 * 613 + 29, 64 * 1200, 800_003])
@pytest.mark.parametrize('deleted', [False, True])
def test_prefix_across_epoch_ends(ops, oracle, monkeypatch, N, deleted):
    """an epoch end after every other step: the prefix in flight at the loop exit is dropped and issued again at the next entry"""
    monkeypatch.setenv('ANNLITE_Q8_TUNE', '1,2,192,3')
    _check(ops, oracle, monkeypatch, N, 41, 10, seed=N % 97, deleted=deleted)


@pytest.mark.parametrize('N', [1, 63, 64 * 15 + 2, 64 * 31 + 63])
def test_prefix_tiny_slices(ops, oracle, monkeypatch, N):
    """slices of a few blocks or less: the prefix of a block past the slice's end is issued and never used"""
    k = min(10, N)
    cb, codes, q = _structured(ops, max(N, 64), 9, seed=N)
    cs = ops.codes_skew(codes[:N])
    d1, i1, _ = _search(ops, monkeypatch, True, q, cb, cs, k)
    d0, i0, _ = _search(ops, monkeypatch, False, q, cb, cs, k)
    assert np.array_equal(d1, d0) and np.array_equal(i1, i0)
    lut = oracle.batch_precompute_adc_table_c(q.cpu().numpy(), 8, 256, cb.cpu().numpy())
    rd, ri = oracle.adc_search_c(lut, ops.codes_to_numpy(codes)[:N], k, threads=oracle.max_threads())
    assert np.array_equal(d1, rd) and np.array_equal(i1, ri)


def test_prefix_with_second_phases_and_rebuilds(ops, oracle, monkeypatch):
    """a rebuild at every epoch end, deleted rows: second phases and epoch ends both drop and re-issue the prefix"""
    monkeypatch.setenv('ANNLITE_Q8_TUNE', '3,2,192,0')
    monkeypatch.setenv('ANNLITE_Q8_TARGET', '64')
    monkeypatch.setenv('ANNLITE_Q8_REBUILD', '7')
    c1 = _check(ops, oracle, monkeypatch, 555_557, 52, 10, seed=13, deleted=True)
    assert c1[2] > 0, c1


def test_prefix_uniform_codes_finish_in_place(ops, oracle, monkeypatch):
    """independent random codes: most steps finish in place (the prefix re-issued after each)"""
    rs = np.random.RandomState(11)
    N, B, k = 90_001, 24, 10
    cb = rs.randn(M, 256, 8).astype(np.float32)
    codes = rs.randint(0, 256, size=(N, M)).astype(np.uint8)
    q = rs.randn(B, M * 8).astype(np.float32)
    cs = ops.codes_skew(ops.to_dev(codes))
    d1, i1, c1 = _search(ops, monkeypatch, True, ops.to_dev(q), ops.to_dev(cb), cs, k)
    d0, i0, _ = _search(ops, monkeypatch, False, ops.to_dev(q), ops.to_dev(cb), cs, k)
    assert c1[3] > 0, c1
    assert np.array_equal(d1, d0) and np.array_equal(i1, i0)
    lut = oracle.batch_precompute_adc_table_c(q, 8, 256, cb)
    rd, ri = oracle.adc_search_c(lut, codes, k, threads=oracle.max_threads())
    assert np.array_equal(d1, rd) and np.array_equal(i1, ri)


@pytest.mark.parametrize('case', ['inf_query', 'nan_query'])
def test_prefix_non_finite_tables(ops, oracle, monkeypatch, case):
    from test_round4_gpu import _nonfinite_inputs

    N, B, Ks, dsub, k = 50_001, 17, 256, 8, 10
    cb, x, q, kind = _nonfinite_inputs(case, M, dsub, N, B, Ks, seed=M * 77 + k)
    codes = oracle.encode_c(x, cb)
    with np.errstate(all='ignore'):
        lut = oracle.batch_precompute_adc_table_c(q, dsub, Ks, cb)
        rd, ri = oracle.adc_search_c(lut, codes, k)
    cs = ops.codes_skew(ops.to_dev(codes))
    d1, i1, _ = _search(ops, monkeypatch, True, ops.to_dev(q), ops.to_dev(cb), cs, k)
    d0, i0, _ = _search(ops, monkeypatch, False, ops.to_dev(q), ops.to_dev(cb), cs, k)
    assert np.array_equal(i1, i0) and np.array_equal(d1, d0, equal_nan=True)
    assert np.array_equal(i1, ri) and np.array_equal(d1, rd, equal_nan=True)


for _name in [n for n in list(globals()) if n.startswith('test_') and n != 'test_next_block_lookups_in_flight_across_the_vote']:
    for _m in gpu:
        globals()[_name] = _m(globals()[_name])
