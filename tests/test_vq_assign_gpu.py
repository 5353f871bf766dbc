"""GPU: ``annlite_vq_assign`` / ``annlite_vq_cell_sums`` (vq.hip) against float64 numpy, and against the cell
selection's chain (``ivf_select_cells`` with one probe), whose answer is the specification bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _assign_both(x, cb):
    """(the new path's cells, the chain's cells, the undecided rows of the new path)"""
    from annlite_amd import ops

    ws = ops.ScanWorkspace()
    xd, cd = ops.to_dev(x), ops.to_dev(cb)
    got = ops.vq_assign(xd, cd, ws).cpu().numpy()
    return got, ops.ivf_select_cells(0, xd, cd, 1)[:, 0].cpu().numpy(), ops.vq_assign_undecided(ws)


# a partial row tile; a second row tile and scalar loads; a partial second centroid block and a K tail; a third block; scalar loads past
# four stages, eight blocks
@pytest.mark.parametrize('N,C,D', [(1, 1, 1), (129, 2, 3), (127, 129, 33), (300, 257, 64), (1000, 1024, 130)])
def test_assign_matches_float64_and_the_chain(N, C, D):
    from annlite_amd.core.codec.vq import vq_assign_slack

    rs = np.random.RandomState(N + C + D)
    x, cb = rs.randn(N, D).astype(np.float32), rs.randn(C, D).astype(np.float32)
    got, chain, undecided = _assign_both(x, cb)
    x64, c64 = x.astype(np.float64), cb.astype(np.float64)
    xn, cn = (x64 * x64).sum(1), (c64 * c64).sum(1)
    d = xn[:, None] + cn[None, :] - 2.0 * (x64 @ c64.T)
    order = np.argsort(d, axis=1, kind='stable')
    best = order[:, 0]
    if C > 1:
        second = order[:, 1]
        gap = d[np.arange(N), second] - d[np.arange(N), best]
        exempt = gap < vq_assign_slack(D, xn, cn[best]).astype(np.float64) + vq_assign_slack(D, xn, cn[second])
    else:
        exempt = np.zeros(N, bool)
    print('exempt %d of %d, undecided %d' % (exempt.sum(), N, undecided))
    assert exempt.mean() <= 0.05
    assert np.array_equal(got[~exempt], best[~exempt])
    assert np.array_equal(got, chain)
    assert 0 <= undecided <= N


def _adversarial(case):
    """(rows, centroids, the undecided rows to expect)"""
    rs = np.random.RandomState(11)
    N, C, D = 200, 130, 16
    x, cb = rs.randn(N, D).astype(np.float32), rs.randn(C, D).astype(np.float32)
    if case == 'identical centroids':  # every score ties: nothing is decided, the chain answers cell 0
        return x, np.repeat(cb[:1], C, 0), N
    if case == 'duplicated pairs':  # cells 2 i and 2 i + 1 are one point: the gap is 0, the lower id wins
        return x, np.repeat(cb[:C // 2], 2, 0), N
    if case == 'rows equal to a centroid':  # a distance of exactly 0 against gaps of about 2 D
        return cb[rs.randint(0, C, N)].copy(), cb, 0
    if case == 'a NaN row':
        x[7, 3] = np.nan
        return x, cb, 1
    if case == 'an inf centroid':  # its score is not finite for any row
        cb[5, 2] = np.inf
        return x, cb, N
    assert case == 'large offset'  # eps ~ 73 u (|x|^2 + |c|^2) ~ 150 against distances of about 0.3: nothing is decided
    return (1000.0 + 0.1 * rs.randn(N, D)).astype(np.float32), (1000.0 + 0.1 * rs.randn(C, D)).astype(np.float32), N


@pytest.mark.parametrize('case', ['identical centroids', 'duplicated pairs', 'rows equal to a centroid', 'a NaN row', 'an inf centroid',
                                  'large offset'])
def test_assign_adversarial_equals_the_chain(case):
    x, cb, expect = _adversarial(case)
    got, chain, undecided = _assign_both(x, cb)
    assert np.array_equal(got, chain)
    assert undecided == expect
    if case == 'identical centroids':
        assert (got == 0).all()
    if case == 'duplicated pairs':
        assert (got % 2 == 0).all()


# two slabs would need D > 64: (5000, 3, 130) has three, the last partial; the last case has cells of 3 chunks, 1 chunk and 0 rows
@pytest.mark.parametrize('N,C,D,long_cell', [(1000, 7, 5, False), (5000, 3, 130, False), (20000, 3, 70, True)])
def test_cell_sums_match_float64_and_repeat(N, C, D, long_cell):
    import torch

    from annlite_amd import ops

    rs = np.random.RandomState(N)
    x = rs.randn(N, D).astype(np.float32)
    cells = rs.randint(0, C, N).astype(np.int32)
    if long_cell:
        cells = np.where(rs.rand(N) < 0.9, 1, 0).astype(np.int32)  # ~18000 rows in cell 1 (chunks of 8192), none in cell 2
    xd, cd = ops.to_dev(x), ops.to_dev(cells)
    sums, counts = ops.vq_cell_sums(xd, cd, C)
    sums2, counts2 = ops.vq_cell_sums(xd, cd, C)
    assert torch.equal(sums, sums2) and torch.equal(counts, counts2)  # (equal as bits: no NaN here)
    assert np.array_equal(counts.cpu().numpy(), np.bincount(cells, minlength=C))
    ref, mag = np.zeros((C, D)), np.zeros((C, D))
    np.add.at(ref, cells, x.astype(np.float64))
    np.add.at(mag, cells, np.abs(x.astype(np.float64)))
    # one f32 rounding of the float64 sum (the two float64 orders differ by far less: N 2^-53 of the magnitudes)
    err = np.abs(sums.cpu().numpy().astype(np.float64) - ref)
    assert (err <= 2.0 ** -24 * np.abs(ref) + N * 2.0 ** -53 * mag).all(), err.max()


def test_seeded_fit_repeats_bit_for_bit():
    from annlite_amd.core.codec.vq import VQCodec

    rs = np.random.RandomState(5)
    x = (rs.randn(32, 16)[rs.randint(0, 32, 4096)] * 3.0 + rs.randn(4096, 16)).astype(np.float32)

    def fit(assign):
        codec = VQCodec(32, iter=25, n_init=2)
        codec.seed, codec.assign = 1234, assign
        codec.fit(x)
        cb = codec.codebook.astype(np.float64)
        return codec.codebook, ((x[:, None, :] - cb[None]) ** 2).sum(2).min(1).sum()

    (cb1, inertia), (cb2, _), (_, chain_inertia) = fit('mfma'), fit('mfma'), fit('chain')
    assert cb1.tobytes() == cb2.tobytes()
    print('inertia (mfma - chain) / chain: %.3e' % ((inertia - chain_inertia) / chain_inertia))
    # The two paths assign alike and differ in the rounding of the update (f64 sums rounded once / f32 atomics in arrival order).
    # Measured on this table at three seeds (scripts/bench_vq_assign.py --fit-spread, profiles/vq_assign/fit_inertia_spread.jsonl):
    # (mfma - chain) / chain = -1.7e-13 .. -2.0e-13, the chain's own run-to-run spread 2.4e-14 .. 4.0e-14.  The bound is five times the
    # larger figure: 1e-12.
    assert inertia <= (1.0 + 1e-12) * chain_inertia
