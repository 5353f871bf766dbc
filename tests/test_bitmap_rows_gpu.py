"""``annlite_bitmap_rows`` ("selected rows"): the set bits of a bitmap as an ascending list of offsets, against
``numpy.flatnonzero`` of the unpacked bits.  Sizes around a word (32 rows), around what one workgroup owns (1024 words = 32768 rows) and
across many workgroups -- once across more than the scan takes in one pass (1024); bits behind the rows, a second bitmap, an output shorter than the selection, and the same array twice."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

SIZES = [1, 31, 32, 33, 4096, 32767, 32768, 32769, 300_001]
PATTERNS = ['zero', 'one', 'last', 'first', 'half', 'sparse', 'run']


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _flags(pattern, N, seed=0):
    rs = np.random.RandomState(seed + N % 1009)
    f = np.zeros(N, dtype=bool)
    if pattern == 'one':
        f[:] = True
    elif pattern == 'last':
        f[N - 1] = True
    elif pattern == 'first':
        f[0] = True
    elif pattern == 'half':
        f = rs.rand(N) < 0.5
    elif pattern == 'sparse':
        f = rs.rand(N) < 0.01
    elif pattern == 'run':  # one dense run in the middle, ragged against words and workgroups
        f[N // 3: N // 3 + max(1, N // 4)] = True
    return f


def _pack(flags, spare_words=0, tail=None):
    """bool [N] -> i32 words (``spare_words`` more behind them); ``tail``: what the bits at positions >= N are set to (bool)"""
    N = len(flags)
    n_words = (N + 31) // 32 + spare_words
    bits = np.zeros(n_words * 32, dtype=bool)
    if tail:
        bits[N:] = True
    bits[:N] = flags
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder='little').view(np.uint32).reshape(-1).view(np.int32)


@pytest.mark.parametrize('N', SIZES)
def test_rows_are_flatnonzero_of_the_bits(ops, N):
    for pattern in PATTERNS:
        flags = _flags(pattern, N)
        want = np.flatnonzero(flags)
        for tail in (False, True):  # bits set behind row N - 1, in the last word and in spare words, must not appear
            words = ops.to_dev(_pack(flags, spare_words=2, tail=tail))
            rows, n = ops.bitmap_rows(words, n_rows=N)
            assert n == len(want), (pattern, N, tail, n, len(want))
            assert rows.dtype.is_floating_point is False and rows.numel() == n
            assert np.array_equal(rows.cpu().numpy(), want), (pattern, N, tail)


@pytest.mark.parametrize('pattern', ['last', 'first', 'sparse'])
def test_more_workgroup_counts_than_the_scan_takes_at_once(ops, pattern):
    """N = 1024 * 32768 + 1: 1025 workgroup counts, so ``bitmap_rows_scan_kernel`` -- 1024 counts per pass -- runs a second pass and carries
    the total of the first into it (300 001 rows are 10 counts: one pass).  The last workgroup owns row N - 1 alone.  Sparse selections
    only: the output stays small."""
    import torch

    WG = 32768
    N = 1024 * WG + 1
    flags = np.zeros(N, dtype=bool)
    if pattern == 'last':
        flags[N - 1] = True
    elif pattern == 'first':
        flags[0] = True
    else:  # about 1000 rows, some of them in the workgroups 0, 1023 and 1024
        rs = np.random.RandomState(7)
        flags[rs.randint(0, N, size=1000)] = True
        flags[[5, WG - 1, 1023 * WG, 1023 * WG + 77, 1024 * WG - 1, N - 1]] = True
    want = np.flatnonzero(flags)
    assert len(want) <= 1006
    for tail in (False, True):
        words = ops.to_dev(_pack(flags, spare_words=2, tail=tail))
        buf = torch.full((2048,), -7, dtype=torch.int32, device=words.device)
        rows, n = ops.bitmap_rows(words, n_rows=N, out=buf)
        assert n == len(want), (pattern, tail, n, len(want))
        got = buf.cpu().numpy()
        assert np.array_equal(got[:n], want) and (got[n:] == -7).all(), (pattern, tail)


@pytest.mark.parametrize('N', [33, 32769, 300_001])
def test_and_bits(ops, N):
    a, b = _flags('half', N, seed=1), _flags('half', N, seed=2)
    for other in (b, _flags('run', N), _flags('zero', N)):
        rows, n = ops.bitmap_rows(ops.to_dev(_pack(a, tail=True)), ops.to_dev(_pack(other, tail=True)), n_rows=N)
        want = np.flatnonzero(a & other)
        assert n == len(want) and np.array_equal(rows.cpu().numpy(), want)


@pytest.mark.parametrize('N', [33, 32769, 300_001])
def test_a_short_output_takes_the_first_rows_and_the_count_is_the_whole(ops, N):
    import torch

    flags = _flags('half', N, seed=3)
    want = np.flatnonzero(flags)
    words = ops.to_dev(_pack(flags))
    for cap in (0, 1, len(want) // 2, len(want) - 1, len(want)):
        buf = torch.full((cap + 64,), -7, dtype=torch.int32, device=words.device)  # (the sentinel: behind `cap`, nothing is written)
        rows, n = ops.bitmap_rows(words, n_rows=N, out=buf[:cap])
        assert n == len(want) and rows.numel() == cap
        got = buf.cpu().numpy()
        assert np.array_equal(got[:cap], want[:cap]) and (got[cap:] == -7).all(), (N, cap)


def test_two_runs_give_the_same_array(ops):
    import torch

    N = 300_001
    words = ops.to_dev(_pack(_flags('half', N, seed=4)))
    first = ops.bitmap_rows(words, n_rows=N)[0].clone()
    again = ops.bitmap_rows(words, n_rows=N)[0]
    assert torch.equal(first, again)


def test_bad_arguments_are_errors(ops):
    words = ops.to_dev(np.zeros(4, np.int32))
    with pytest.raises(Exception):
        ops.bitmap_rows(words, n_rows=4 * 32 + 1)  # more rows than the words hold
