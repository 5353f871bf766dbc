"""The byte-table kernel's split step (``adc_scan_q8_kernel<16, 16, true, 2, 1, true, 16, false, 12>``, scan_q8.hip): a step adds 12
of the 16 sub-spaces, drops the rows whose partial byte sum already fails every slot's bound, and runs the full test over the
survivors 64 at a time.  ``ANNLITE_Q8_SPLIT=0`` is the one-phase step.  Both must return the same bits, and the oracle's."""
import os

import numpy as np
import pytest

from conftest import has_gpu

M = 16
gpu = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs an AMD GPU')]


def test_partial_sums_never_drop_a_row_the_full_test_keeps():
    """CPU: the filter's byte arithmetic on partial sums -- S_h <= S for entries >= 0, so a slot that fails on S_h fails on S"""
    rs = np.random.RandomState(0)
    for _ in range(200):
        q = rs.randint(0, 16, size=(64, M, 4)).astype(np.uint32)  # 64 rows, 16 sub-spaces, 4 queries per dword
        T = rs.randint(0, 128, size=4).astype(np.uint32)
        th = np.uint32(0)
        for b in range(4):
            th |= np.uint32((0x80 | int(T[b])) << (8 * b))

        def hits(S):  # the kernel's test of four byte sums packed in a dword
            sm = np.zeros(len(S), np.uint32)
            for b in range(4):
                sm |= (S[:, b] << (8 * b)).astype(np.uint32)
            return ((th - (sm & np.uint32(0x7f7f7f7f))) & ~sm & np.uint32(0x80808080)).astype(np.uint32)

        full = hits(q.sum(axis=1))
        for h in (8, 10, 12):
            part = hits(q[:, :h].sum(axis=1))
            assert np.all((full & ~part) == 0), h  # every bit the full test keeps is kept by the partial one


def _bits(valid):
    bits = np.zeros(((len(valid) + 31) // 32 + 2) * 32, dtype=bool)
    bits[:len(valid)] = valid
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder='little').view(np.int32).reshape(-1)


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _search(ops, monkeypatch, split, q, cb, codes_skewed, k, valid_bits=None):
    import torch
    from annlite_amd import _capi
    from annlite_amd._capi import LUT_L2

    monkeypatch.setenv('ANNLITE_SCAN_VARIANT', '50')
    monkeypatch.setenv('ANNLITE_DEBUG_COUNTERS', '1')
    if split:
        monkeypatch.delenv('ANNLITE_Q8_SPLIT', raising=False)
    else:
        monkeypatch.setenv('ANNLITE_Q8_SPLIT', '0')
    _capi.knobs_reload()
    try:
        d, i = ops.pq_search_topk(LUT_L2, q, cb, codes_skewed, k, M, 256, codes_layout=1, valid_bits=valid_bits)
        torch.cuda.synchronize()
        cnt = _capi.debug_split_counters()
    finally:
        monkeypatch.delenv('ANNLITE_DEBUG_COUNTERS')
        monkeypatch.delenv('ANNLITE_Q8_SPLIT', raising=False)
        _capi.knobs_reload()
    return d.cpu().numpy(), i.cpu().numpy(), cnt


def _structured(ops, N, B, seed):
    from test_k64_byte_tables import _structured as s

    return s(ops, N, B, 8, seed)


@pytest.mark.parametrize('N,B,k', [(2_100_037, 100, 10), (300_001, 45, 16), (64 * 700 + 5, 33, 1)])
@pytest.mark.parametrize('deleted', [False, True])
def test_split_step_equals_the_one_phase_step_and_the_oracle(ops, oracle, monkeypatch, N, B, k, deleted):
    """structured data (the bench's model): epoch ends at 2M rows, a row count that is not a multiple of 64, deleted rows"""
    cb, codes, q = _structured(ops, N, B, seed=N % 997 + k)
    valid = np.ones(N, bool)
    vb = None
    if deleted:
        valid[np.random.RandomState(k).choice(N, N // 10, replace=False)] = False
        vb = ops.to_dev(_bits(valid))
    cs = ops.codes_skew(codes)
    d1, i1, c1 = _search(ops, monkeypatch, True, q, cb, cs, k, vb)
    d0, i0, c0 = _search(ops, monkeypatch, False, q, cb, cs, k, vb)
    assert c1[0] > 0 and c1[1] > 0 and c1[2] > 0, c1  # the split step ran: rows through phase one, survivors, second-phase steps
    assert c0 == [0, 0, 0, 0], c0
    assert c1[1] < c1[0] // 4, c1  # (structured data: most rows fail on 12 sub-spaces)
    assert np.array_equal(d1, d0) and np.array_equal(i1, i0)
    nq = min(B, 8)
    lut = oracle.batch_precompute_adc_table_c(q[:nq].cpu().numpy(), 8, 256, cb.cpu().numpy())
    live = np.nonzero(valid)[0]
    rd, ri = oracle.adc_search_c(lut, ops.codes_to_numpy(codes)[live], k, threads=oracle.max_threads())
    assert np.array_equal(d1[:nq], rd) and np.array_equal(i1[:nq], live[ri])


def test_uniform_codes_take_the_fallback(ops, oracle, monkeypatch):
    """independent random codes: most rows survive, the steps finish in place"""
    import torch

    rs = np.random.RandomState(5)
    N, B, k = 150_000, 40, 10
    cb = rs.randn(M, 256, 8).astype(np.float32)
    codes = rs.randint(0, 256, size=(N, M)).astype(np.uint8)
    q = rs.randn(B, M * 8).astype(np.float32)
    cb_d, q_d = ops.to_dev(cb), ops.to_dev(q)
    cs = ops.codes_skew(ops.to_dev(codes))
    d1, i1, c1 = _search(ops, monkeypatch, True, q_d, cb_d, cs, k)
    d0, i0, _ = _search(ops, monkeypatch, False, q_d, cb_d, cs, k)
    assert np.array_equal(d1, d0) and np.array_equal(i1, i0)
    lut = oracle.batch_precompute_adc_table_c(q, 8, 256, cb)
    rd, ri = oracle.adc_search_c(lut, codes, k, threads=oracle.max_threads())
    assert np.array_equal(d1, rd) and np.array_equal(i1, ri)
    torch.cuda.synchronize()


def test_forced_rebuilds(ops, oracle, monkeypatch):
    """an epoch end every other step and a rebuild as soon as a bound moves: the survivor rings are drained at every end"""
    monkeypatch.setenv('ANNLITE_Q8_TUNE', '1,2,192,0')
    monkeypatch.setenv('ANNLITE_Q8_TARGET', '64')
    monkeypatch.setenv('ANNLITE_Q8_REBUILD', '7')
    N, B, k = 400_003, 48, 10
    cb, codes, q = _structured(ops, N, B, seed=23)
    cs = ops.codes_skew(codes)
    d1, i1, c1 = _search(ops, monkeypatch, True, q, cb, cs, k)
    d0, i0, _ = _search(ops, monkeypatch, False, q, cb, cs, k)
    assert c1[2] > 0, c1
    assert np.array_equal(d1, d0) and np.array_equal(i1, i0)
    lut = oracle.batch_precompute_adc_table_c(q.cpu().numpy(), 8, 256, cb.cpu().numpy())
    rd, ri = oracle.adc_search_c(lut, ops.codes_to_numpy(codes), k, threads=oracle.max_threads())
    assert np.array_equal(d1, rd) and np.array_equal(i1, ri)


@pytest.mark.parametrize('case', ['inf_query', 'nan_query', 'huge_codewords_some'])
def test_non_finite_tables(ops, oracle, monkeypatch, case):
    from test_round4_gpu import _nonfinite_inputs

    N, B, Ks, dsub, k = 70_000, 21, 256, 8, 10
    cb, x, q, kind = _nonfinite_inputs(case, M, dsub, N, B, Ks, seed=M * 100 + k)
    codes = oracle.encode_c(x, np.where(np.isfinite(cb), cb, 0).astype(np.float32) if case.startswith('huge') else cb)
    with np.errstate(all='ignore'):
        lut = oracle.batch_precompute_adc_table_c(q, dsub, Ks, cb)
        rd, ri = oracle.adc_search_c(lut, codes, k)
    cs = ops.codes_skew(ops.to_dev(codes))
    d1, i1, _ = _search(ops, monkeypatch, True, ops.to_dev(q), ops.to_dev(cb), cs, k)
    assert np.array_equal(i1, ri) and np.array_equal(d1, rd, equal_nan=True)


for _name in [n for n in list(globals()) if n.startswith('test_') and n != 'test_partial_sums_never_drop_a_row_the_full_test_keeps']:
    for _m in gpu:
        globals()[_name] = _m(globals()[_name])
