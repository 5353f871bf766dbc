"""Every index class over the shared row store (annlite_amd/core/index/row_store.py), on the GPU: a table grown in three adds from
``initial_size=64`` in steps of 64 (two growths, each batch crossing 32-row bitmap words), with ten rows overwritten and five deleted,
answers bit for bit like the same class filled in ONE add at its final capacity -- at ``limit`` 10, 65 (the large-k path) and 250
(more than the rows), with and without an ``indices=`` filter that straddles word boundaries, and again after ``dump`` -> ``load``.

Codebooks (and the coarse centroids) are the golden fixtures', as in test_gpu_parity.py / test_ivf.py.

Two classes set limits of their own, kept as they are:
  * ``IvfPQGpuIndex`` with ``n_probe < n_cells`` refuses ``limit > 64`` (asserted below); limits 65 and 250 run with ``n_probe=n_cells``.
  * ``HnswPQGpuIndex`` refuses ``update_with_ids`` (asserted below) and, with the graph built on the GPU, takes ids in insertion
    order only: nothing is overwritten there, and the one-add twin adds all 200 rows and deletes the same five.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR, has_gpu, load_golden

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs an AMD GPU')]

N = 200
BATCHES = ((0, 50), (50, 150), (150, 200))
OVERWRITTEN = np.array([1, 30, 33, 49, 50, 95, 96, 149, 150, 198])
DELETED = [31, 32, 63, 64, 199]
SURVIVORS = np.setdiff1d(np.arange(N), DELETED)
FILTER = np.array([0, 5, 30, 31, 32, 33, 62, 63, 64, 65, 96, 127, 128, 160, 198, 199])
LIMITS = (10, 65, 250)
CASES = ['flat', 'flat_cosine', 'pq_skewed', 'pq_plain', 'ivf', 'hnsw']


def _case(case):
    """(factory(initial_size), rows [N + 10, D], queries, search(idx, x, limit, indices))"""
    import torch

    from annlite_amd import Metric, PQCodec
    from annlite_amd.core.codec.vq import VQCodec
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.core.index.hnsw_pq_gpu import HnswPQGpuIndex
    from annlite_amd.core.index.ivf_pq_gpu import IvfPQGpuIndex
    from annlite_amd.core.index.pq_flat_gpu import PQFlatGpuIndex

    search = lambda idx, x, limit, indices: idx.search_batch(x, limit=limit, indices=indices)  # noqa: E731
    if case == 'ivf':
        z = np.load(os.path.join(GOLDEN_DIR, 'cells', 'cells_m16_d64.npz'))
        M, dsub, Ks, C = int(z['meta'][0]), int(z['meta'][1]), int(z['meta'][2]), int(z['meta'][5])
        codec = PQCodec(dim=M * dsub, n_subvectors=M, n_clusters=Ks, metric=Metric.EUCLIDEAN)
        codec.set_codebooks(torch.from_numpy(z['codebooks']))
        vq = VQCodec(C, metric=Metric.EUCLIDEAN)
        vq._codebook, vq._is_trained = z['centroids'], True
        make = lambda size: IvfPQGpuIndex(dim=M * dsub, metric=Metric.EUCLIDEAN, pq_codec=codec, vq_codec=vq, n_probe=4,  # noqa: E731
                                          initial_size=size, expand_step_size=64)
        # (the pruned search takes limit <= 64; beyond, every cell is visited)
        search = lambda idx, x, limit, indices: idx.search_batch(x, limit=limit, indices=indices,  # noqa: E731
                                                                 n_probe=None if limit <= 64 else C)
        return make, z['x'][:N + 10], z['queries'], search
    g = load_golden('c2_m16_d128')
    kw = dict(dim=g['D'], initial_size=None, expand_step_size=64)
    if case.startswith('flat'):
        metric = Metric.COSINE if case == 'flat_cosine' else Metric.EUCLIDEAN
        make = lambda size: FlatGpuIndex(**{**kw, 'initial_size': size}, metric=metric)  # noqa: E731
    else:
        codec = PQCodec(dim=g['D'], n_subvectors=g['M'], n_clusters=g['Ks'], metric=Metric.EUCLIDEAN).set_codebooks(g['codebooks'])
        if case == 'hnsw':
            make = lambda size: HnswPQGpuIndex(**{**kw, 'initial_size': size}, metric=Metric.EUCLIDEAN, pq_codec=codec)  # noqa: E731
            search = lambda idx, x, limit, indices: idx.search_exhaustive(x, limit=limit, indices=indices)  # noqa: E731
        else:
            make = lambda size: PQFlatGpuIndex(**{**kw, 'initial_size': size}, metric=Metric.EUCLIDEAN, pq_codec=codec,  # noqa: E731
                                               skewed=case == 'pq_skewed')
    return make, g['x'][:N + 10], g['queries'], search


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _answers(idx, search, q):
    return {(limit, filtered): search(idx, q, limit, FILTER if filtered else None) for limit in LIMITS for filtered in (False, True)}


def _same(got, want):
    for key, (d, i) in got.items():
        assert isinstance(d, np.ndarray) and isinstance(i, np.ndarray), key  # numpy in gives numpy out
        assert d.dtype == np.float32 and i.dtype == np.int64 and d.shape == i.shape == want[key][0].shape, key
        assert np.array_equal(i, want[key][1]), key
        assert np.array_equal(_bits(d), _bits(want[key][0])), key


@pytest.mark.parametrize('case', CASES)
def test_grown_overwritten_deleted_table_equals_the_one_add_table(case, tmp_path):
    import torch

    torch.cuda.set_device(0)
    make, rows, q, search = _case(case)
    x = rows[:N].copy()
    # ---- the table under test: three adds, two growths; ten overwrites; five deletes
    idx = make(64)
    assert idx.capacity == 64 and idx.size == 0
    for n, (a, b) in enumerate(BATCHES):
        idx.add_with_ids(x[a:b], np.arange(a, b))
        assert (idx.size, idx.capacity, idx._n_rows) == (b, (64, 192, 256)[n], b)
    if case == 'hnsw':
        with pytest.raises(RuntimeError):
            idx.update_with_ids(rows[N:], OVERWRITTEN)
    else:
        x[OVERWRITTEN] = rows[N:]
        idx.update_with_ids(rows[N:], OVERWRITTEN)
    assert (idx.size, idx.capacity, idx._n_rows) == (N, 256, N)
    idx.delete(DELETED)
    idx.delete([63])  # (deleted already: counts nothing)
    assert (idx.size, idx.capacity, idx._n_rows) == (N - 5, 256, N)
    with pytest.raises(AssertionError):
        idx.add_with_ids(x[:2], [-1, 3])  # a negative id: refused by every index before anything is written
    assert (idx.size, idx._n_rows) == (N - 5, N)
    # ---- its twin: one add at the final capacity
    twin = make(256)
    if case == 'hnsw':
        twin.add_with_ids(x, np.arange(N))
        twin.delete(DELETED)
    else:
        twin.add_with_ids(x[SURVIVORS], SURVIVORS)
    assert (twin.size, twin.capacity) == (N - 5, 256)
    want = _answers(twin, search, q)
    # ---- the shape of the twin's own answers: what is compared below is not empty
    live = SURVIVORS if case != 'ivf' else None
    for (limit, filtered), (d, i) in want.items():
        assert d.shape == i.shape == (q.shape[0], limit)
        pool = np.intersect1d(FILTER, SURVIVORS) if filtered else SURVIVORS
        real = i >= 0
        assert np.isin(i[real], pool).all() and np.isinf(d[~real]).all() and (d[~real] > 0).all()
        assert (np.diff(real.astype(np.int8), axis=1) <= 0).all()  # the missing places trail
        if live is not None or limit > 64:  # (every row is visited: the answer holds all it may)
            assert (real.sum(axis=1) == min(limit, len(pool))).all(), (limit, filtered)
        assert all(len(set(r[r >= 0])) == (r >= 0).sum() for r in i)
    if case == 'ivf':
        with pytest.raises(AssertionError):
            idx.search_batch(q, limit=65)
    _same(_answers(idx, search, q), want)
    # ---- tensors stay tensors
    qd = torch.from_numpy(q).cuda()
    for filtered in (False, True):
        d, i = search(idx, qd, 10, FILTER if filtered else None)
        td, ti = search(twin, qd, 10, FILTER if filtered else None)
        assert isinstance(d, torch.Tensor) and isinstance(i, torch.Tensor) and d.is_cuda and i.is_cuda
        assert d.dtype == torch.float32 and i.dtype == torch.int64
        assert torch.equal(i, ti) and torch.equal(d.view(torch.int32), td.view(torch.int32))
    # ---- search(): one query, valid entries only, `limit` clipped to the filter
    lim = {'ivf': 10, 'hnsw': 10}.get(case, 250)  # (the pruned search and the graph walk set limits of their own: not this file's subject)
    d, i = idx.search(q[0], limit=lim)
    assert isinstance(d, np.ndarray) and d.shape == i.shape and d.ndim == 1 and (i >= 0).all() and np.isin(i, SURVIVORS).all()
    assert np.isfinite(d).all()
    if case != 'ivf':
        assert len(i) == min(lim, N - 5)
    d, i = idx.search(q[0], limit=10, indices=[5, 31, 32])
    assert d.shape == i.shape and set(i.tolist()) <= {5} and (case == 'ivf' or i.tolist() == [5])
    # ---- dump -> load into a fresh, smaller object
    p = tmp_path / 'index.bin'
    idx.dump(p)
    again = make(64)
    again.load(p)
    assert (again.size, again.capacity, again._n_rows) == (N - 5, 256, N)
    assert torch.equal(again._valid, idx._valid) and torch.equal(again._valid_bool, idx._valid_bool)
    _same(_answers(again, search, q), want)


@pytest.mark.parametrize('case', ['flat', 'pq_skewed', 'pq_plain'])
def test_files_with_the_first_formats_keys_load(case, tmp_path):
    """A dict written by hand with exactly the keys and the format string of the files from before the row store existed."""
    import torch

    from annlite_amd import Metric, ops

    torch.cuda.set_device(0)
    make, rows, q, search = _case(case)
    x = rows[:N]
    valid = np.zeros(N, bool)
    valid[SURVIVORS] = True
    state = {'dim': x.shape[1], 'metric': int(Metric.EUCLIDEAN), 'n_rows': N, 'size': N - 5, 'capacity': 256, 'valid': valid}
    # (capacity: a multiple of the writer's step that holds its n_rows -- a file never says less -- and more than the loader's own 64)
    twin = make(256)
    twin.add_with_ids(x[SURVIVORS], SURVIVORS)
    if case == 'flat':
        state.update(format='annlite_amd.FlatGpuIndex/1', vectors=x)
        assert len(state) == 8
    else:
        codes = ops.codes_to_numpy(ops.pq_encode(ops.to_dev(x), twin.pq_codec.codebooks_dev))
        state.update(format='annlite_amd.PQFlatGpuIndex/1', M=twin.M, Ks=twin.Ks, codes=codes, vectors=None)
        assert len(state) == 11
    p = tmp_path / 'old.bin'
    with open(p, 'wb') as f:
        np.save(f, np.array([state], dtype=object), allow_pickle=True)
    idx = make(64)
    idx.load(p)
    assert (idx.size, idx.capacity, idx._n_rows) == (N - 5, 256, N)
    _same(_answers(idx, search, q), _answers(twin, search, q))
    # ... and today's files hold the same keys
    idx.dump(tmp_path / 'new.bin')
    assert set(np.load(tmp_path / 'new.bin', allow_pickle=True)[0]) == set(state)
