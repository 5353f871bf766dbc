"""numpy references shared by the kernel test files (not a conftest, no pytest setting): the NaN-last order with ties by id,
the oracle's top-k over arbitrary (distance, id) pairs, the SKEWED code layout, the key of a float, the validity bitmap.  Each is
itself checked without a GPU, against the oracle or a brute-force loop, in tests/test_post_scan_kernels.py and
tests/test_ivf_stage_kernels.py."""
import numpy as np
import pytest

from conftest import has_gpu

gpu = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs an AMD GPU')]


def on_gpu(f):
    for m in gpu:
        f = m(f)
    return f


def bits(*words):
    return np.array(words, dtype=np.uint32).view(np.float32)


NANS = bits(0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0xffc12345)  # both signs, quiet / signalling, payloads
SUBNORMALS = bits(0x00000001, 0x80000001, 0x007fffff, 0x807fffff)


def lexsort_nan_last(vals, ids):
    """Permutation that sorts (vals, ids) ascending in numpy's order with ties by id: numbers by value (-0.0 == +0.0), then
    every NaN, each group by id."""
    vals = np.asarray(vals, dtype=np.float32)
    nan = np.isnan(vals)
    return np.lexsort((np.asarray(ids), np.where(nan, np.float32(0), vals), nan))


def topk_pairs(oracle, vals, ids, k):
    """The oracle's top-k over (distance, id) pairs with arbitrary distinct ids: pairs put in id order, so that the oracle's
    tie-break (position) IS the id.  Returns (f32 [k], i64 [k]) padded with (+inf, -1)."""
    vals, ids = np.asarray(vals, dtype=np.float32), np.asarray(ids, dtype=np.int64)
    by_id = np.argsort(ids, kind='stable')
    d, pos = oracle.top_k_c(vals[by_id], k)
    return d, np.where(pos >= 0, ids[by_id][np.clip(pos, 0, max(ids.size - 1, 0))] if ids.size else -1, -1)


def topk_pairs_numpy(vals, ids, k):
    """The same through the NaN-last lexsort (second, independent statement)."""
    vals, ids = np.asarray(vals, dtype=np.float32), np.asarray(ids, dtype=np.int64)
    o = lexsort_nan_last(vals, ids)[:k]
    pad = k - o.size
    return (np.concatenate([vals[o], np.full(pad, np.inf, np.float32)]), np.concatenate([ids[o], np.full(pad, -1, np.int64)]))


def skew_rows(plain, ids, inverse=False):
    """SKEWED storage of PLAIN rows: byte j of row n = code of sub-space (j + n) mod M; M = 64: two 32-byte
    halves, each rotated by n mod 32, and a byte whose position p = j mod 32 has p + n mod 32 >= 32 stores code - 1 (mod 256).
    ``inverse``: ``plain`` holds stored rows, the PLAIN rows come back."""
    plain = np.asarray(plain, dtype=np.uint8)
    ids = np.asarray(ids, dtype=np.int64)
    M = plain.shape[1]
    j = np.arange(M)[None, :]
    if M == 64:
        r = (ids % 32)[:, None]
        h, p = j // 32, j % 32
        if not inverse:
            src = 32 * h + (p + r) % 32
            return (np.take_along_axis(plain, src, axis=1).astype(np.int64) - (p + r >= 32)).astype(np.uint8)
        ps = (p - r) % 32                           # stored position (inside its half) of sub-space j
        return (np.take_along_axis(plain, 32 * h + ps, axis=1).astype(np.int64) + (ps + r >= 32)).astype(np.uint8)
    r = (ids % M)[:, None]
    return np.take_along_axis(plain, (j + r) % M if not inverse else (j - r) % M, axis=1)


def f32_key(v):
    """The lists' distance key (common.h): order-preserving image of the float's bits, every NaN 0xffc00000 (behind +inf)."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    u = v.view(np.uint32).astype(np.uint64)
    k = (u ^ np.where(u >> np.uint64(31), np.uint64(0xffffffff), np.uint64(0x80000000))) & np.uint64(0xffffffff)
    return np.where(np.isnan(v), np.uint64(0xffc00000), k)


def bitmap(valid):
    """bool [N] -> the validity bitmap i32 [ceil(N / 32) + 2], bit n % 32 of word n / 32"""
    N = valid.size
    b = np.zeros(((N + 31) // 32 + 2) * 32, bool)
    b[:N] = valid
    return np.packbits(b.reshape(-1, 32), axis=1, bitorder='little').view(np.int32).reshape(-1)
