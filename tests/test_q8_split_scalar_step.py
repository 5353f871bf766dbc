"""The split step's per-block bookkeeping (``adc_scan_q8_kernel<..., HS>``, HS > 0, scan_q8.hip: load_block, split_step, shq_v).

What a step knows per WAVE is kept off the VALU: the next block's code rows and validity word are fetched from a scalar base
(SALU next to blk_row) plus a lane offset; the vote compares the 32-bit popcount in SALU; the debug counter of the rows through
phase one sits behind a scalar branch; the block counter, the bias words and the survivor ring are addressed from one VGPR with
immediate offsets (no SGPR kept in a VGPR lane is read in the common trip); and the loop runs two blocks per trip, the two sets of
row registers in swapped roles, so that no step copies the next rows over the current ones.  Nothing about which rows are
tested, or in what order, changes: results are bit-identical.

CPU: the ISA of the common trip, per block.  VALU instructions from a block's first instruction to its vote's branch (the draw's
`ds_add_rtn` included, which the parent's loop rotation kept in front of the window):

    HS = 11:  parent 77 (+ 3 for the draw in front of the window), now 68        HS = 12:  parent 78 (+ 3), now 69

that is the look-ups' own 64 (65) plus 4: the two lane offsets' clamps (`v_min_u32`, `v_cndmask_b32`: the per-lane clamp to the
table's last row is a minimum with a scalar per load -- taken on a uniform branch instead, each side's offset cost a `v_mov`
for the same count) and the validity test (`v_and_b32`, `v_cmp_ne_u32`).  The ceilings below are these numbers.

GPU: the places where the new addressing, the clamp and the two-block trip matter -- tables smaller than a block, last blocks,
slice ends in mid-block with and without a bitmap, epoch ends after every other block with odd and even block counts,
interleaved slices, steps that finish in place from both halves of a trip, the debug counters -- against the one-phase step
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

PARENT_VALU = {11: 77, 12: 78}
VALU_CEILING = {11: 68, 12: 69}  # the look-ups' 64 (65 at HS = 12) plus 4
# the one-phase step of the same shape (HS = 0): its step loop is the parent's, counted on the parent commit
HS0_LOOP = {'valu': 146, 'lds': 38, 'vmem': 2, 'instructions': 284}
SYM = '_ZN7annlite18adc_scan_q8_kernelILi16ELi16ELb1ELi2ELi1ELb1ELi16ELb0ELi%dEEEvNS_8ScanArgsE'


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


def _loop(lines, hs):
    """(instructions, labels) of the step loop: labels[j] = the basic-block label in front of instruction j, if any"""
    sym = SYM % hs
    i0 = next(j for j, ln in enumerate(lines) if ln.startswith(sym + ':'))
    i1 = next(j for j in range(i0, len(lines)) if lines[j].lstrip().startswith('.amdhsa_kernel ' + sym))
    ins, labels = [], {}
    for ln in _step_loop(lines[i0:i1]):
        m = re.match(r'^\.L(BB\d+_\d+):', ln)
        if m:
            labels[len(ins)] = m.group(1)
        elif ln.startswith('\t') and not ln.lstrip().startswith((';', '.')):
            ins.append(ln.strip())
    return ins, labels


def _blocks(ins):
    """The common trip, block by block: [(first, vote_branch, end)] index ranges into ins.  A block starts at the loop header or
    behind the previous block's v_readfirstlane of the drawn block number, fetches its next code rows with the ONE
    global_load_dwordx4 that has an SGPR base (the rare parts' loads take a 64-bit VGPR address: `off`), votes at the first
    s_bcnt1_i32_b64 behind that, and ends with the v_readfirstlane of its draw."""
    rows = [j for j, ln in enumerate(ins) if re.match(r'global_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\]', ln)]
    out, first = [], 0
    for r in rows:
        pop = next(j for j in range(r, len(ins)) if ins[j].startswith('s_bcnt1_i32_b64'))
        vote = next(j for j in range(pop, len(ins)) if ins[j].startswith('s_cbranch'))
        end = next(j for j in range(vote, len(ins)) if ins[j].startswith('v_readfirstlane_b32'))
        out.append((first, vote, end))
        first = end + 1
    return out


@pytest.mark.parametrize('hs', [11, 12])
def test_common_trip_keeps_per_block_bookkeeping_off_the_valu(asm_lines, hs):
    ins, labels = _loop(asm_lines, hs)
    blocks = _blocks(ins)
    assert len(blocks) == 2, (hs, blocks, 'two blocks per trip: one SGPR-base code-row load each')
    # no scalar memory load and no 64-bit VALU compare anywhere in the step loop, its rare parts included
    assert not [ln for ln in ins if ln.startswith(('s_load', 's_buffer_load'))], hs
    assert not [ln for ln in ins if re.match(r'v_cmp\w*_[ui]64', ln)], hs
    assert not [ln for ln in ins if 'scratch_' in ln], hs
    for n, (first, vote, end) in enumerate(blocks):
        head = ins[first:vote + 1]
        n_valu = sum(ln.startswith('v_') for ln in head)
        print('HS = %d, block %d of a trip: %d VALU instructions to the vote (parent: %d)' % (hs, n, n_valu, PARENT_VALU[hs]))
        assert n_valu <= VALU_CEILING[hs], (hs, n, n_valu, [ln for ln in head if ln.startswith('v_')])
        # the look-ups themselves are all there
        assert sum(ln.startswith('ds_read_b128') for ln in head) == 2 * hs, (hs, n)
        assert sum(ln.startswith('v_perm_b32') for ln in head) == hs, (hs, n)
        # the vote: scalar compares on the popcount
        assert [ln for ln in ins[vote + 1:end] if re.match(r's_cmp_\w+_u32', ln)], (hs, n)
        # the whole block of the common trip -- header, vote, survivor store, the bounds' refresh, the draw's broadcast: the code
        # row from an SGPR base, the validity word a vector load too, no SGPR read back from a VGPR lane, no register copies
        trip = ins[first:end + 1]
        assert sum(ln.startswith('global_load_dwordx4') for ln in trip) == 1, (hs, n)
        word = [ln for ln in trip if ln.startswith('global_load_dword ')]
        assert len(word) == 1 and re.search(r', v\d+, s\[\d+:\d+\]', word[0]), (hs, n, word)
        assert not [ln for ln in trip if ln.startswith(('v_readlane', 'v_writelane'))], (hs, n)
        assert sum(ln.startswith('v_readfirstlane') for ln in trip) == 1, (hs, n)
        assert not [ln for ln in trip if re.match(r'v_mov_b32_e32 v\d+, v\d+', ln)], (hs, n, 'a register copy per step')
        # the step waits for no load it has just issued (tests/test_q8_split_row_wait.py, in both halves of the trip)
        first_lookup = next(j for j, ln in enumerate(trip) if ln.startswith('ds_read_b128'))
        issued = 0
        for ln in trip[:first_lookup]:
            issued += ln.startswith('global_load')
            m = re.match(r's_waitcnt\s+vmcnt\((\d+)\)', ln)
            assert not m or int(m.group(1)) >= issued, (hs, n, ln)
        assert issued == 2, (hs, n, issued)
    # the second block's code runs into the back edge or the loop's exit without passing a rare part: the blocks are laid out
    # back to back (the rare parts out of line behind them)
    assert blocks[1][0] == blocks[0][2] + 1


def test_one_phase_step_loop_is_the_parents(asm_lines):
    ins, _ = _loop(asm_lines, 0)
    got = {'valu': sum(ln.startswith('v_') for ln in ins), 'lds': sum(ln.startswith('ds_') for ln in ins),
           'vmem': sum(ln.startswith(('global_', 'buffer_')) for ln in ins), 'instructions': len(ins)}
    assert got == HS0_LOOP, got


# ------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _bitmap(N, seed):
    """N mod 32 != 0 is the caller's; 20 % of the rows deleted, one whole 64-row block deleted, the last block partly deleted"""
    rs = np.random.RandomState(seed)
    valid = np.ones(N, bool)
    valid[rs.choice(N, N // 5, replace=False)] = False
    if N >= 3 * 64:
        b = (N // 64) // 2
        valid[64 * b:64 * b + 64] = False
    last = 64 * ((N - 1) // 64)
    valid[last:] = True
    valid[last:N:2] = False
    valid[N - 1] = True
    return valid


def _check(ops, oracle, monkeypatch, N, B, k, seed, valid=None, data=None, counters=None):
    cb, codes, q = data if data is not None else _structured(ops, N, B, seed=seed)
    vb = ops.to_dev(_bits(valid)) if valid is not None else None
    if valid is None:
        valid = np.ones(N, bool)
    cs = ops.codes_skew(codes)
    d1, i1, c1 = _search(ops, monkeypatch, True, q, cb, cs, k, vb)
    d0, i0, c0 = _search(ops, monkeypatch, False, q, cb, cs, k, vb)
    assert c1[0] > 0 and c0 == [0, 0, 0, 0], (c1, c0)  # (the split step ran, and only where asked)
    assert np.array_equal(d1, d0) and np.array_equal(i1, i0)
    nq = min(B, 8)
    lut = oracle.batch_precompute_adc_table_c(q[:nq].cpu().numpy(), 8, 256, cb.cpu().numpy())
    live = np.nonzero(valid)[0]
    kk = min(k, len(live))
    rd, ri = oracle.adc_search_c(lut, ops.codes_to_numpy(codes)[live], kk, threads=oracle.max_threads())
    assert np.array_equal(d1[:nq, :kk], rd) and np.array_equal(i1[:nq, :kk], live[ri])
    if counters is not None:
        counters.append(c1)
    return c1


@pytest.mark.parametrize('N', [1, 63, 64, 65, 64 * 15 + 2, 64 * 31 + 63])
@pytest.mark.parametrize('deleted', [False, True])
def test_last_block_and_tables_below_one_block(ops, oracle, monkeypatch, N, deleted):
    """the clamp to the table's last row: a table smaller than one block, a last block of 1, 2, 63 and 64 rows"""
    valid = None
    if deleted and N > 1:
        valid = np.ones(N, bool)
        valid[::3] = False
        valid[N - 1] = True
    _check(ops, oracle, monkeypatch, N, 9, 1 if N < 10 else 10, seed=N, valid=valid)


@pytest.mark.parametrize('N', [64 * 613 + 29, 64 * 1200, 800_003])
@pytest.mark.parametrize('bitmap', [False, True])
def test_slice_ends_in_mid_block(ops, oracle, monkeypatch, N, bitmap):
    """a ragged tile (B = 41), slices that end inside a block; with a bitmap (N mod 32 != 0 or a whole number of blocks) and without"""
    _check(ops, oracle, monkeypatch, N, 41, 10, seed=N % 89, valid=_bitmap(N, 7) if bitmap else None)


@pytest.mark.parametrize('N', [64 * (2 * 260 + 1) * 1 + 17, 64 * 2 * 260, 64 * 777 + 1])
@pytest.mark.parametrize('bitmap', [False, True])
def test_epoch_end_after_every_other_block(ops, oracle, monkeypatch, N, bitmap):
    """ANNLITE_Q8_TUNE=1,2,192,3: epochs end after every other block, odd and even numbers of blocks per slice -- a two-block trip
    leaves after its first half, and the rows fetched ahead move to where the next epoch picks them up"""
    monkeypatch.setenv('ANNLITE_Q8_TUNE', '1,2,192,3')
    _check(ops, oracle, monkeypatch, N, 37, 10, seed=N % 101, valid=_bitmap(N, 11) if bitmap else None)


@pytest.mark.parametrize('bitmap', [False, True])
def test_interleaved_slices(ops, oracle, monkeypatch, bitmap):
    """ANNLITE_Q8_ILV: a slice is runs of blocks that are not contiguous -- the scalar base is made from the block number every time"""
    monkeypatch.setenv('ANNLITE_Q8_ILV', '3')
    N = 555_557
    _check(ops, oracle, monkeypatch, N, 33, 10, seed=3, valid=_bitmap(N, 5) if bitmap else None)


@pytest.mark.parametrize('N', [64 * 40 + 9, 64 * 41 + 9])
def test_uniform_codes_finish_in_place_from_both_halves(ops, oracle, monkeypatch, N):
    """independent random codes: most steps finish in place, odd and even block counts enter the rare parts from both halves of a trip"""
    rs = np.random.RandomState(N)
    B, k = 24, 10
    cb = rs.randn(M, 256, 8).astype(np.float32)
    codes = rs.randint(0, 256, size=(N, M)).astype(np.uint8)
    q = rs.randn(B, M * 8).astype(np.float32)
    data = (ops.to_dev(cb), ops.to_dev(codes), ops.to_dev(q))
    c1 = _check(ops, oracle, monkeypatch, N, B, k, seed=0, data=data)
    assert c1[3] > 0, c1  # steps finished in place


@pytest.mark.parametrize('bitmap', [False, True])
def test_debug_counters(ops, oracle, monkeypatch, bitmap):
    """annlite_debug_split_counters with the first one behind its scalar branch: rows through phase one = (valid rows) x (query
    tiles) -- every valid row of every tile goes through the first phase exactly once.  The other three are consistent: a
    second-phase wave-step takes 64 survivors from its wave's ring, except the one short step with which a wave empties its ring
    at an epoch end, so survivors >= 64 (second-phase steps - drains).  The drains are per WAVE and epoch, not per slice (15
    scanning waves a work item, each with a ring of its own), so the count used is the most the plan admits: 15 waves x work
    items x 8 epoch ends (ends after steps 15, 255, 4095, ...: fewer than 8 for any table of < 2^32 rows)."""
    from annlite_amd._capi import scan_plan

    N, B, k = 64 * 901 + 37, 70, 10  # (B = 70: three query tiles of 32)
    valid = _bitmap(N, 13) if bitmap else None
    c1 = _check(ops, oracle, monkeypatch, N, B, k, seed=17, valid=valid)
    n_valid = int(valid.sum()) if bitmap else N
    tiles = (B + 31) // 32
    items = scan_plan(N, M, 256, 1, B, k).n_slices * tiles
    print('split counters %s, valid rows x tiles %d, work items %d' % (c1, n_valid * tiles, items))
    assert c1[0] == n_valid * tiles, (c1, n_valid, tiles)
    assert min(c1) >= 0 and 0 < c1[1] <= c1[0] and c1[2] > 0, c1
    assert c1[1] >= 64 * (c1[2] - 15 * items * 8), (c1, items)
    assert c1[2] <= c1[1] // 64 + 15 * items * 8 and c1[3] <= tiles * ((N + 63) // 64), (c1, items)


for _name in [n for n in list(globals()) if n.startswith('test_') and n not in (
        'test_common_trip_keeps_per_block_bookkeeping_off_the_valu', 'test_one_phase_step_loop_is_the_parents')]:
    for _m in gpu:
        globals()[_name] = _m(globals()[_name])
