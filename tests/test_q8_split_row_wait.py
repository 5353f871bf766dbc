"""The split step (``adc_scan_q8_kernel<..., 12>``, scan_q8.hip) fetches the next block's code rows and validity word one step ahead.
The rows fetched in front of the step loop (the first block of a work item, the next block across an epoch end) are waited for
there, so that the loop header's wait state holds no pending load: with them pending, every step waited with vmcnt(1) for the
row it had just issued.  The CPU test pins that in the ISA; the GPU tests run the places where the
rows cross that wait -- epoch ends after every other step, ragged row counts, the last block of a slice, deleted rows, forced
rebuilds -- against the one-phase step and the oracle."""
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import has_gpu
from test_isa_step_loop import _step_loop
from test_q8_split_step import _bits, _search, _structured

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'annlite_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
gpu = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs an AMD GPU')]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not installed')
def test_split_step_does_not_wait_for_the_row_it_just_issued():
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, 'scan_q8.s')
        cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-mllvm',
               '-amdgpu-atomic-optimizer-strategy=None', '-S', '--cuda-device-only', 'scan_q8.hip', '-o', asm]
        subprocess.run(cmd, cwd=CSRC, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=900)
        lines = open(asm).read().splitlines()
    # the split step of the plain search: M = 16, SKEWED rows, row queue, 16-key lists, HS = 12
    sym = '_ZN7annlite18adc_scan_q8_kernelILi16ELi16ELb1ELi2ELi1ELb1ELi16ELb0ELi12EEEvNS_8ScanArgsE'
    i0 = next(j for j, ln in enumerate(lines) if ln.startswith(sym + ':'))
    i1 = next(j for j in range(i0, len(lines)) if lines[j].lstrip().startswith('.amdhsa_kernel ' + sym))
    window = _step_loop(lines[i0:i1])
    ins = [ln.strip() for ln in window if ln.startswith('\t') and not ln.lstrip().startswith((';', '.'))]
    first_lookup = next(j for j, ln in enumerate(ins) if ln.startswith('ds_read_b128'))
    issued = 0
    for ln in ins[:first_lookup]:
        if ln.startswith('global_load'):
            issued += 1
        m = re.match(r's_waitcnt\s+vmcnt\((\d+)\)', ln)
        if m:
            # a wait for fewer than `issued` outstanding loads waits for one the step has just issued for the next step
            assert int(m.group(1)) >= issued, (ln, issued, 'the step waits for the code row it fetches for the next step')
    assert issued >= 2, issued  # (the code row and the validity word: the loop found is the step loop)


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
        valid[rs.choice(N, N // 7, replace=False)] = False
        valid[-70:] = False  # (the last block of the table: partly deleted, partly live)
        valid[-3] = True
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


@pytest.mark.parametrize('N', [64 * 977 + 63, 64 * 1500, 500_001])
@pytest.mark.parametrize('deleted', [False, True])
def test_epoch_end_every_other_step(ops, oracle, monkeypatch, N, deleted):
    """epochs end after every other step (rows fetched across an end are waited for at the next loop entry), ragged and whole slices"""
    monkeypatch.setenv('ANNLITE_Q8_TUNE', '1,2,192,3')
    _check(ops, oracle, monkeypatch, N, 37, 10, seed=N % 101, deleted=deleted)


@pytest.mark.parametrize('deleted', [False, True])
def test_forced_rebuilds_with_deleted_rows(ops, oracle, monkeypatch, deleted):
    """a rebuild at every epoch end (every 4th step), deleted rows and a partly deleted last block"""
    monkeypatch.setenv('ANNLITE_Q8_TUNE', '3,2,192,0')
    monkeypatch.setenv('ANNLITE_Q8_TARGET', '64')
    monkeypatch.setenv('ANNLITE_Q8_REBUILD', '7')
    _check(ops, oracle, monkeypatch, 333_333, 48, 10, seed=41, deleted=deleted)


@pytest.mark.parametrize('N', [64 * 15 + 1, 64 * 2 + 17])
def test_fewer_blocks_than_waves(ops, oracle, monkeypatch, N):
    """a slice of one or two blocks per wave at most: the rows fetched before the loop are the only ones"""
    _check(ops, oracle, monkeypatch, N, 20, 10, seed=N, deleted=True)


for _name in [n for n in list(globals()) if n.startswith('test_') and n != 'test_split_step_does_not_wait_for_the_row_it_just_issued']:
    for _m in gpu:
        globals()[_name] = _m(globals()[_name])
