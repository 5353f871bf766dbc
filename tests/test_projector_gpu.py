"""The PCA projector on the GPU: ``annlite_affine_rows`` and ``annlite_pca_accumulate`` against float64
numpy under their derived bounds, ``ProjectorCodec.fit`` / ``partial_fit`` against sklearn's float64 PCA on planted data, and
``AnnLite(n_components=K, projector='gpu')`` in front of the flat, PQ, cells and graph indexes.

The bounds (u = 2^-24; an MFMA output element is one k-ordered f32 fma chain, the textbook any-order bound is gamma_k; the factor
2 covers the MFMA's internal accumulation):
  affine_rows     |err|       <= 2 (Din + 2) u (|x - sub| |M|^T + |add|)       (one subtraction, Din fma steps, one addition)
  pca_accumulate  |dG_ij|     <= 2 (n + 2) u sum_r |x_ri - s_i| |x_rj - s_j|   against float64 sums of the f32 differences
                  |dsum_i|    <= 2 (n + 2) u sum_r |x_ri - s_i|
"""
import numpy as np
import pytest

from _projector_data import IDS, SHAPES, U24, gaps, planted, signed_cosines
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


# ---------------------------------------------------------------------------------------------------------------- affine_rows
def _strided(ops, a, ld, fill):
    """``a`` [n, d] as a view of a device buffer with row stride ``ld`` whose padding columns hold ``fill``."""
    import torch

    full = torch.full((a.shape[0], ld), fill, dtype=torch.float32, device=ops.device())
    full[:, : a.shape[1]] = ops.to_dev(a)
    return full, full[:, : a.shape[1]]


def _misaligned(ops, a):
    """``a`` [n, d] on the device starting 4 bytes past a 16-byte boundary."""
    import torch

    buf = torch.empty((a.size + 1,), dtype=torch.float32, device=ops.device())
    buf[1:] = ops.to_dev(a).reshape(-1)
    v = buf[1:].view(a.shape)
    assert v.data_ptr() % 16 == 4
    return v


AFFINE_CASES = [
    # n, Din, Dout, options
    (1, 1, 1, {}),
    (127, 3, 8, {}),
    (128, 31, 127, {}),
    (129, 32, 128, {}),
    (300, 33, 129, {}),
    (300, 100, 8, dict(ldx=108, ldo=11)),      # row strides beyond the rows (16-byte path): the padding of out stays untouched
    (129, 100, 127, dict(ldx=101, ldo=127)),   # an odd row stride: the scalar loads
    (129, 130, 129, dict(sub=False, add=False)),
    (127, 31, 8, dict(misaligned=True)),       # Din % 4 != 0 on a row start that is not 16-byte aligned
    (128, 32, 1, dict(misaligned=True)),       # Din % 4 == 0, but the pointer is not: the scalar loads too
    (300, 130, 128, {}),
    (1, 130, 129, {}),
    (300, 32, 8, dict(sub=False)),
    (127, 33, 127, dict(add=False)),
    # fewer than 512 (128-row tile, output tile) pairs are served in 32-row tiles -- every shape above; from 512 on in 128-row tiles:
    (65408, 32, 8, {}),                        # 511 row tiles: the last shape in 32-row tiles
    (65409, 32, 127, {}),                      # 512: the first in 128-row tiles (16-byte loads)
    (65409, 31, 8, dict(misaligned=True)),     # ... scalar loads, an odd row length, the last tile one row long
    (65409, 100, 8, dict(ldx=108, ldo=11)),
    (65409, 33, 1, {}),
    (32700, 130, 129, dict(sub=False, add=False)),  # two output tiles: 256 row tiles suffice
]


@pytest.mark.parametrize('n,Din,Dout,opt', AFFINE_CASES, ids=[f'{c[0]}x{c[1]}to{c[2]}' + ''.join('-' + k for k in c[3]) for c in AFFINE_CASES])
def test_affine_rows_within_the_derived_bound(ops, n, Din, Dout, opt):
    import torch

    rs = np.random.RandomState(n * 1000 + Din * 10 + Dout)
    x = (50.0 + rs.randn(n, Din)).astype(np.float32)  # a common offset that `sub` removes before the products
    M = rs.randn(Dout, Din).astype(np.float32)
    sub = (50.0 + 0.1 * rs.randn(Din)).astype(np.float32) if opt.get('sub', True) else None
    add = (3.0 * rs.randn(Dout)).astype(np.float32) if opt.get('add', True) else None
    if opt.get('misaligned'):
        xd, x_full = _misaligned(ops, x), None
    elif 'ldx' in opt:
        x_full, xd = _strided(ops, x, opt['ldx'], 1e30)  # (padding that would wreck every sum it entered)
    else:
        xd = ops.to_dev(x)
    Md = ops.to_dev(M)
    sd = None if sub is None else ops.to_dev(sub)
    ad = None if add is None else ops.to_dev(add)
    outs = []
    for _ in range(2):
        if 'ldo' in opt:
            out_full = torch.full((n, opt['ldo']), -7.0, dtype=torch.float32, device=xd.device)
            got = ops.affine_rows(xd, Md, sub=sd, add=ad, out=out_full[:, :Dout])
            torch.cuda.synchronize()
            assert bool((out_full[:, Dout:] == -7.0).all()), 'padding columns of out were written'
        else:
            got = ops.affine_rows(xd, Md, sub=sd, add=ad)
            torch.cuda.synchronize()
        assert got.shape == (n, Dout) and got.dtype == torch.float32
        outs.append(got.cpu().numpy().copy())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), 'two runs differ'
    t = x.astype(np.float64) - (0.0 if sub is None else sub.astype(np.float64))
    a64 = np.zeros(Dout) if add is None else add.astype(np.float64)
    want = t @ M.astype(np.float64).T + a64
    bound = 2.0 * (Din + 2) * U24 * (np.abs(t) @ np.abs(M.astype(np.float64)).T + np.abs(a64))
    err = np.abs(outs[0].astype(np.float64) - want)
    print('max err / bound', float((err / bound).max()))
    assert (err <= bound).all(), (float((err / bound).max()), np.argwhere(err > bound)[:5])


def test_affine_rows_of_no_rows(ops):
    import torch

    M = ops.to_dev(np.ones((8, 32), np.float32))
    out = ops.affine_rows(torch.empty((0, 32), dtype=torch.float32, device=M.device), M, sub=ops.to_dev(np.ones(32, np.float32)))
    assert out.shape == (0, 8)
    with pytest.raises(AssertionError):
        ops.affine_rows(torch.empty((4, 31), dtype=torch.float32, device=M.device), M)


# ---------------------------------------------------------------------------------------------------------------- pca_accumulate
def _accumulate(ops, batches, s):
    import torch

    D = s.shape[0]
    dev = ops.device()
    sum64 = torch.zeros((D,), dtype=torch.float64, device=dev)
    gram64 = torch.zeros((D, D), dtype=torch.float64, device=dev)
    sd = ops.to_dev(s)
    for b in batches:
        ops.pca_accumulate(ops.to_dev(b), sd, sum64, gram64)
    torch.cuda.synchronize()
    return sum64.cpu().numpy(), gram64.cpu().numpy()


def _check_accumulate(x, s, got_sum, got_gram):
    n = x.shape[0]
    t = (x - s).astype(np.float32).astype(np.float64)  # the f32 subtraction the kernel performs, then exact sums
    gram, ssum = t.T @ t, t.sum(axis=0)
    bg = 2.0 * (n + 2) * U24 * (np.abs(t).T @ np.abs(t))
    bs = 2.0 * (n + 2) * U24 * np.abs(t).sum(axis=0)
    eg, es = np.abs(got_gram - gram), np.abs(got_sum - ssum)
    print('gram err / bound', float((eg / bg).max()), 'sum err / bound', float((es / bs).max()))
    assert (eg <= bg).all(), float((eg / bg).max())
    assert (es <= bs).all(), float((es / bs).max())
    assert np.array_equal(got_gram, got_gram.T), 'the Gram matrix handed to _finalize is not symmetric'


def _pca_cases(chunk):
    return [(1, 1), (2, 3), (chunk - 1, 31), (chunk, 32), (chunk + 1, 33), (3 * chunk + 7, 130), (3 * chunk + 7, 1), (1, 130), (chunk + 1, 3),
            (chunk, 130), (2, 32), (chunk - 1, 33), (chunk + 1, 260),  # (260: three column tiles, six tile pairs)
            (17 * chunk + 5, 33)]  # (beyond the 16 chunks whose partials the workspace holds: a second pass)


@pytest.mark.parametrize('case', range(14))
def test_pca_accumulate_within_the_derived_bound(ops, case):
    n, D = _pca_cases(ops.pca_chunk_rows())[case]
    rs = np.random.RandomState(7 * n + D)
    x = (10.0 + rs.randn(n, D) * (1.0 + np.arange(D) % 5)).astype(np.float32)
    s = (10.0 + 0.05 * rs.randn(D)).astype(np.float32)
    got_sum, got_gram = _accumulate(ops, [x], s)
    _check_accumulate(x, s, got_sum, got_gram)
    again = _accumulate(ops, [x], s)
    assert np.array_equal(again[0], got_sum) and np.array_equal(again[1], got_gram), 'two runs differ'


@pytest.mark.parametrize('n1,n2,D', [(700, 900, 130), (3, 513, 33), (512, 1, 32)])
def test_pca_accumulate_over_a_split_batch(ops, n1, n2, D):
    rs = np.random.RandomState(n1 + n2 + D)
    x = (rs.randn(n1 + n2, D) - 4.0).astype(np.float32)
    s = x[:100].mean(axis=0, dtype=np.float32)
    got_sum, got_gram = _accumulate(ops, [x[:n1], x[n1:]], s)
    _check_accumulate(x, s, got_sum, got_gram)  # the float64 truth of the union, the bound of n1 + n2 rows


def test_pca_accumulate_rejects_what_it_cannot_serve(ops):
    import torch

    dev = ops.device()
    x = torch.zeros((4, 2049), dtype=torch.float32, device=dev)
    with pytest.raises(AssertionError):
        ops.pca_accumulate(x, torch.zeros(2049, device=dev), torch.zeros(2049, dtype=torch.float64, device=dev),
                           torch.zeros((2049, 2049), dtype=torch.float64, device=dev))


# ---------------------------------------------------------------------------------------------------------------- fit / partial_fit
CAP = 1.2e-6  # |C_gpu - C_64|_2 / lambda_1: 16 x the largest value an f32 numpy stand-in reaches on the four shapes (7.3e-8)


def _check_model(codec, p):
    """Davis-Kahan: every component within 2 |C_gpu - C_64|_2 / gap_i of sklearn's, with sklearn's sign; |C_gpu - C_64|_2 capped."""
    from annlite_amd.core.codec.projector import _finalize

    K, pca = p['K'], p['pca']
    m = _finalize(codec._n, codec._shift.cpu().numpy(), codec._sum.cpu().numpy(), codec._gram.cpu().numpy(), K)
    assert np.array_equal(m['components'], codec.components)
    dC = np.linalg.norm(m['covariance'] - p['cov64'], 2)
    rel = dC / pca.explained_variance_[0]
    print('|C_gpu - C_64|_2 / lambda_1 =', rel)
    assert rel <= CAP, rel
    cos = signed_cosines(codec.components, pca.components_)
    assert (cos > 0).all(), 'signs differ from sklearn'
    unit = codec.components / np.linalg.norm(codec.components, axis=1, keepdims=True)
    resid = unit - np.sum(unit * pca.components_, axis=1, keepdims=True) * pca.components_
    sin = np.linalg.norm(resid, axis=1)
    lim = 2.0 * dC / gaps(p['lam'], K) + 1e-9
    print('max sin / limit', float((sin / lim).max()))
    assert (sin <= lim).all(), (sin / lim).max()
    np.testing.assert_allclose(codec.explained_variance, pca.explained_variance_, rtol=0, atol=dC + 1e-12)  # (Weyl)
    # the mean is shift + sum / n: the sum's bound over n
    s = codec._shift.cpu().numpy().astype(np.float64)
    lim_mean = 2.0 * (p['N'] + 2) * U24 * np.abs(p['x64'] - s).mean(axis=0) + 1e-12
    assert (np.abs(codec.mean - pca.mean_) <= lim_mean).all()
    return dC


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_fit_finds_sklearns_components(ops, shape):
    from annlite_amd.core.codec.projector import ProjectorCodec

    p = planted(*shape)
    codec = ProjectorCodec(p['D'], n_components=p['K'])
    codec.fit(p['x32'])
    assert codec.is_trained and codec._n == p['N']
    _check_model(codec, p)
    z = codec.encode(p['x32'][:50])
    assert isinstance(z, np.ndarray) and z.shape == (50, p['K']) and z.dtype == np.float32
    zt = codec.encode(ops.to_dev(p['x32'][:50]))
    assert zt.is_cuda and np.array_equal(zt.cpu().numpy(), z)
    # a second fit starts from nothing
    codec.fit(p['x32'])
    assert codec._n == p['N']


@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[2]], ids=[IDS[1], IDS[2]])
def test_partial_fit_in_uneven_batches_is_the_fit_of_the_union(ops, shape):
    """... and decode(encode(x)) is float64 ``inverse_transform(transform(x))`` of the model the codec holds (its float32 mean and
    components in sklearn's float64 PCA object) within the affine_rows bound applied twice: the first bound carried through the
    second map, plus the second map's own."""
    import copy

    from annlite_amd.core.codec.projector import ProjectorCodec

    p = planted(*shape)
    N, D, K, x = p['N'], p['D'], p['K'], p['x32']
    cuts = [0, K + 5, N // 2 + 3, N]
    codec = ProjectorCodec(D, n_components=K)
    for a, b in zip(cuts[:-1], cuts[1:]):
        codec.partial_fit(x[a:b])
        assert codec.is_trained  # after the first call, as in the reference
    assert codec._n == N
    dC_parts = _check_model(codec, p)
    whole = ProjectorCodec(D, n_components=K)
    whole.fit(x)
    dC_whole = _check_model(whole, p)
    # the same components as the fit of the union: both covariances lie within their dC of C_64, so within the sum of each other
    cos = signed_cosines(codec.components, whole.components)
    sin = np.sqrt(np.maximum(0.0, 1.0 - cos * cos))
    assert (cos > 0).all() and (sin <= 2.0 * (dC_parts + dC_whole) / gaps(p['lam'], K) + 1e-7).all(), sin.max()

    xs = x[:300]
    z = codec.encode(xs)
    y = codec.decode(z)
    assert z.shape == (300, K) and y.shape == (300, D) and y.dtype == np.float32
    W = codec.components.astype(np.float32).astype(np.float64)  # what the kernels are given
    mean = codec.mean.astype(np.float32).astype(np.float64)
    ref = copy.deepcopy(p['pca'])
    ref.components_, ref.mean_ = W, mean
    x64 = xs.astype(np.float64)
    z64 = ref.transform(x64)
    y64 = ref.inverse_transform(z64)
    b1 = 2.0 * (D + 2) * U24 * (np.abs(x64 - mean) @ np.abs(W).T)
    ez = np.abs(z.astype(np.float64) - z64)
    assert (ez <= b1).all(), (ez / b1).max()
    b2 = b1 @ np.abs(W) + 2.0 * (K + 2) * U24 * ((np.abs(z64) + b1) @ np.abs(W) + np.abs(mean))
    ey = np.abs(y.astype(np.float64) - y64)
    print('encode err / bound', float((ez / b1).max()), 'decode(encode) err / bound', float((ey / b2).max()))
    assert (ey <= b2).all(), (ey / b2).max()
    # against sklearn's own fit of the same rows (its model differs from the codec's by the fit's error: reported, not bounded here)
    print('max |decode(encode(x)) - sklearn|', float(np.abs(y - p['pca'].inverse_transform(p['pca'].transform(x64))).max()))


def test_whiten_scales_the_components(ops):
    """``whiten=True``: encode with W / sqrt(lambda), decode with W sqrt(lambda) -- the affine bound against float64 on the float32
    matrices the kernels are given, unit variance of the projected training rows, and the same round trip as without."""
    from annlite_amd.core.codec.projector import ProjectorCodec

    p = planted(*SHAPES[0])
    D, K, x = p['D'], p['K'], p['x32']
    plain, white = ProjectorCodec(D, n_components=K), ProjectorCodec(D, n_components=K, whiten=True)
    plain.fit(x)
    white.fit(x)
    assert np.array_equal(plain.components, white.components)  # (the same fit, bit for bit)
    z = white.encode(x)
    scale = np.sqrt(white.explained_variance)[:, None]
    enc = (white.components / scale).astype(np.float32).astype(np.float64)
    dec = (white.components * scale).T.astype(np.float32).astype(np.float64)  # [D, K]
    mean = white.mean.astype(np.float32).astype(np.float64)
    t = x.astype(np.float64) - mean
    z64 = t @ enc.T
    b1 = 2.0 * (D + 2) * U24 * (np.abs(t) @ np.abs(enc).T)
    assert (np.abs(z - z64) <= b1).all()
    # unit variance: w C_64 w^T / lambda_gpu differs from 1 by at most |C_gpu - C_64|_2 / lambda_K <= CAP lambda_1 / lambda_K = 9.6e-6 here,
    # plus the float32 rounding of the matrix (4 u)
    assert np.allclose(z64.var(axis=0, ddof=1), 1.0, rtol=0, atol=1e-5)
    y = white.decode(z)
    y64 = z64 @ dec.T + mean
    b2 = b1 @ np.abs(dec).T + 2.0 * (K + 2) * U24 * ((np.abs(z64) + b1) @ np.abs(dec).T + np.abs(mean))
    assert (np.abs(y - y64) <= b2).all()
    assert np.allclose(y, plain.decode(plain.encode(x)), rtol=0, atol=float(b2.max()) * 4)


# ---------------------------------------------------------------------------------------------------------------- facade
N_DIM, K_DIM = 32, 8


@pytest.fixture(scope='module')
def rows():
    rs = np.random.RandomState(11)
    basis = rs.randn(12, N_DIM) * (2.0 ** -np.arange(12))[:, None] * 4.0
    make = lambda n: (rs.randn(n, 12) @ basis + 0.01 * rs.randn(n, N_DIM) + 0.5).astype(np.float32)  # noqa: E731
    train, x = make(600), make(500)
    q = np.concatenate([x[:8], make(8)]).astype(np.float32)
    return train, x, q


def _docs(x, first=0):
    from annlite_amd.index import Document, DocumentArray

    return DocumentArray([Document(id=str(first + i), embedding=v) for i, v in enumerate(x)])


def _ann(path, **kw):
    from annlite_amd import AnnLite

    return AnnLite(N_DIM, n_components=K_DIM, projector='gpu', data_path=path, **kw)


def _bare_flat(ops, codec, metric, x, q, k):
    """The projected rows in a plain FlatGpuIndex, asked the projected queries: device tensors in, as the facade hands them on."""
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.enums import Metric

    idx = FlatGpuIndex(K_DIM, metric=Metric.from_string(metric), initial_size=len(x))
    idx.add_with_ids(codec.encode(ops.to_dev(x)), np.arange(len(x)))
    d, i = idx.search_batch(codec.encode(ops.to_dev(q)), limit=k)
    return d.cpu().numpy(), i.cpu().numpy()


@pytest.mark.parametrize('metric', ['euclidean', 'cosine'])
def test_facade_flat_float_index_behind_the_projector(ops, rows, tmp_path, metric):
    train, x, q = rows
    ann = _ann(tmp_path, metric=metric)
    assert not ann.is_trained
    ann.train(train)
    assert ann.is_trained and ann._projector_codec_path.exists() and ann.vec_index(0).dim == K_DIM
    ann.index(_docs(x))
    assert ann.index_size == 500 and ann.get_doc_by_id('3').embedding.shape == (N_DIM,)  # documents keep their embeddings
    d, i = ann.search_numpy(q, limit=10)
    d, i = np.stack(d), np.stack(i)
    bd, bi = _bare_flat(ops, ann._projector_codec, metric, x, q, 10)
    assert d.dtype == np.float32 and np.array_equal(i, bi) and np.array_equal(d.view(np.uint32), bd.view(np.uint32))
    assert np.array_equal(i[:8, 0], np.arange(8)), 'a stored vector does not find itself first'
    dists, matches = ann.search_by_vectors(q[:2], limit=3)
    assert [m.id for m in matches[0]] == [str(v) for v in i[0, :3]]

    ann.dump()
    again = _ann(tmp_path, metric=metric)  # reopened: the projector and the rows come from the files, nothing is trained
    assert again.is_trained and again.index_size == 500
    d2, i2 = again.search_numpy(q, limit=10)
    assert np.array_equal(np.stack(i2), i) and np.array_equal(np.stack(d2).view(np.uint32), d.view(np.uint32))

    # update: new embeddings under old ids; delete
    moved = (x[100:103] + 1.0).astype(np.float32)
    ann.update(_docs(moved, first=100))
    ann.delete(['7'])
    assert ann.total_docs == 499 and ann.index_size == 499
    d3, i3 = ann.search_numpy(np.concatenate([moved, x[7:8]]), limit=5)
    assert [int(r[0]) for r in i3[:3]] == [100, 101, 102] and 7 not in i3[3].tolist()


def test_facade_pq_index_behind_the_projector(ops, rows, tmp_path):
    train, x, q = rows
    ann = _ann(tmp_path, n_subvectors=4, n_clusters=32, metric='euclidean')
    assert ann._pq_codec.dim == K_DIM and not ann.is_trained
    ann.train(train)
    assert ann.is_trained and ann._pq_codec.is_trained and ann._pq_codec.codebooks.shape == (4, 32, 2)
    ann.index(_docs(x))
    d, i = ann.search_numpy(q, limit=10)
    assert len(d) == 16 and all(len(r) == 10 for r in i) and all((np.diff(r) >= 0).all() for r in d)
    codes = ann.encode(x[:20])
    assert codes.shape == (20, 4)
    back = ann.decode(codes)
    assert back.shape == (20, N_DIM) and back.dtype == np.float32
    # the round trip is the PQ codec's approximation inside the projected space, carried back: closer to x than the mean is
    mean = ann._projector_codec.mean.astype(np.float32)
    assert np.linalg.norm(back - x[:20]) < np.linalg.norm(mean[None, :] - x[:20])
    # partial_train: the projector first, then the other codecs through it
    pt = _ann(tmp_path / 'pt', n_subvectors=4, n_clusters=32, metric='euclidean')
    for a in range(0, 600, 200):  # (force_train as in the reference's own loop, index.py:181: the index is trained after the first batch)
        pt.partial_train(train[a:a + 200], force_train=True)
    assert pt.is_trained and pt._projector_codec._n == 600


@pytest.mark.parametrize('kind', ['cells', 'graph'])
def test_facade_cells_and_graph_over_projected_floats_equal_the_flat_index(ops, rows, tmp_path, kind):
    from annlite_amd.core.index.hnsw_flat_gpu import HnswFlatGpuIndex
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex

    train, x, q = rows
    if kind == 'cells':  # every cell probed: the exact answer over all rows
        ann = _ann(tmp_path, metric='euclidean', n_cells=4, n_probe=4, ivf_prune=True)
        assert isinstance(ann.vec_index(0), IvfFlatGpuIndex)
    else:  # (the walk's list as long as the kernel allows: over 500 rows it holds every neighbour that matters)
        ann = _ann(tmp_path, metric='euclidean', graph=True, build='gpu', ef_search=256)
        assert isinstance(ann.vec_index(0), HnswFlatGpuIndex)
    assert ann.vec_index(0).dim == K_DIM
    ann.train(train)
    assert ann.is_trained
    ann.index(_docs(x))
    d, i = ann.search_numpy(q, limit=10)
    bd, bi = _bare_flat(ops, ann._projector_codec, 'euclidean', x, q, 10)
    assert np.array_equal(np.stack(i), bi) and np.array_equal(np.stack(d).view(np.uint32), bd.view(np.uint32))
