"""The row store the GPU indexes share (annlite_amd/core/index/row_store.py) and the result helpers above it, on the CPU: a toy
subclass with two columns lives on ``cpu`` through the ``_device()`` hook; nothing here touches a GPU or loads the library."""
import numpy as np
import pytest
import torch

from annlite_amd.core.index.row_store import (RowStoreIndex, empty_answer, float_from_key, float_order_key, like_input, pad_to_k,
                                              ranked_answer, take_by_position)
from annlite_amd.enums import Metric


# ------------------------------------------------------------------ the float-order key
def _floats():
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF812345, 0x7FFFFFFF], dtype=np.uint32).view(np.float32)
    vals = np.array([3.5, -2.0, 3.5, 0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, -2.0, 0.0, 3.4e38, -3.4e38, np.inf, -0.0, 7.25],
                    dtype=np.float32)
    x = np.concatenate([vals, nans, vals[::-1], nans[::-1]])
    return x[np.random.RandomState(5).permutation(x.size)]


def test_key_orders_floats_like_a_stable_numpy_sort():
    x = _floats()
    key = float_order_key(torch.from_numpy(x) + 0.0)
    assert key.dtype == torch.int64 and int(key.min()) >= -2 ** 31 and int(key.max()) < 2 ** 31
    order = torch.argsort((key << 32) | torch.arange(x.size)).numpy()
    assert np.array_equal(order, np.argsort(x, kind='stable'))


def test_key_keeps_minus_zero_in_front_of_plus_zero():
    key = float_order_key(torch.tensor([-0.0, 0.0]))
    assert int(key[0]) < int(key[1])
    assert int(float_order_key(torch.tensor([np.inf]))[0]) < int(float_order_key(torch.tensor([np.nan]))[0])


def test_key_inverse_returns_the_bits_and_one_nan():
    x = _floats()
    back = float_from_key(float_order_key(torch.from_numpy(x))).numpy()
    assert back.dtype == np.float32
    nan = np.isnan(x)
    assert np.array_equal(back[~nan].view(np.uint32), x[~nan].view(np.uint32))
    assert set(back[nan].view(np.uint32).tolist()) == {int(np.array([np.nan], np.float32).view(np.uint32)[0])}
    # (through the high half of an i64 key as well: what the indexes decode)
    key = (float_order_key(torch.from_numpy(x)) << 32) | 12345
    assert np.array_equal(float_from_key(key >> 32).numpy().view(np.uint32), back.view(np.uint32))


# ------------------------------------------------------------------ bitmap words
def _np_pack(flags):
    return np.packbits(np.asarray(flags).reshape(-1, 32), axis=1, bitorder='little').view(np.uint32).reshape(-1)


def test_pack_and_unpack_bits():
    flags = np.random.RandomState(3).rand(5 * 32) < 0.5
    flags[31], flags[63], flags[95], flags[159] = True, False, True, True  # bit 31 of words 0, 2, 4 set, of word 1 clear
    words = RowStoreIndex._pack_bits(torch.from_numpy(flags))
    assert words.dtype == torch.int32 and words.shape == (5,)
    assert (words.numpy()[[0, 2, 4]] < 0).all() and words.numpy()[1] >= 0
    assert np.array_equal(words.numpy().view(np.uint32), _np_pack(flags))
    for n in (160, 159, 97, 32, 1, 0):
        got = RowStoreIndex._unpack_bits(words, n)
        assert got.dtype == torch.bool and np.array_equal(got.numpy(), flags[:n])


# ------------------------------------------------------------------ result pieces
def test_empty_answer_and_padding():
    d, i = empty_answer(3, 4, torch.device('cpu'))
    assert d.shape == i.shape == (3, 4) and d.dtype == torch.float32 and i.dtype == torch.int64 and d.device.type == 'cpu'
    assert torch.isinf(d).all() and (d > 0).all() and (i == -1).all()
    assert empty_answer(0, 5, 'cpu')[0].shape == (0, 5)
    d0 = torch.tensor([[1.0, 2.0], [3.0, 4.0]], dtype=torch.float64)
    i0 = torch.tensor([[7, 8], [9, 10]], dtype=torch.int32)
    d, i = pad_to_k(d0, i0, 5)
    assert d.shape == i.shape == (2, 5) and d.dtype == torch.float64 and i.dtype == torch.int32
    assert torch.equal(d[:, :2], d0) and torch.equal(i[:, :2], i0) and torch.isinf(d[:, 2:]).all() and (i[:, 2:] == -1).all()
    same = pad_to_k(d0, i0, 2)
    assert same[0] is d0 and same[1] is i0


def test_take_by_position_blanks_missing_and_infinite_places():
    ids = torch.tensor([[10, 11, 12, 13], [20, 21, 22, 23]])
    pos = torch.tensor([[2, 0, -1], [3, 1, 0]])
    d = torch.tensor([[0.5, np.inf, 4.0], [-np.inf, np.nan, 2.0]])
    i = take_by_position(ids, pos, d)
    assert i.dtype == torch.int64 and i.tolist() == [[12, -1, -1], [-1, 21, 20]]  # (NaN is a real row's distance: its id stays)
    rd, ri = ranked_answer(ids, torch.tensor([[4.0, 9.0, np.inf], [1.0, 16.0, 25.0]]), pos, 5, sqrt=True)
    assert rd.tolist() == [[2.0, 3.0, np.inf, np.inf, np.inf], [1.0, 4.0, 5.0, np.inf, np.inf]]
    assert ri.tolist() == [[12, 10, -1, -1, -1], [23, 21, 20, -1, -1]]
    rd, _ = ranked_answer(ids, torch.tensor([[4.0, 9.0, np.inf], [1.0, 16.0, 25.0]]), pos, 3, sqrt=False)
    assert rd.tolist() == [[4.0, 9.0, np.inf], [1.0, 16.0, 25.0]]


def test_like_input():
    d, i = torch.ones((1, 2)), torch.zeros((1, 2), dtype=torch.int64)
    a, b = like_input(True, d, i)
    assert isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == np.float32 and b.dtype == np.int64
    assert like_input(False, d, i) == (d, i)


# ------------------------------------------------------------------ a toy store: the flat index's columns and file, in torch on cpu
class ToyIndex(RowStoreIndex):
    FORMAT = 'annlite_amd.FlatGpuIndex/1'
    STATE_KEYS = ('dim', 'metric')
    ready = True

    def _device(self):
        return torch.device('cpu')

    def _check_ready(self):
        if not self.ready:
            raise RuntimeError('not ready')

    def _columns(self):
        return {'_vectors': ((self.dim,), torch.float32), '_norms': ((), torch.float32)}

    def _write_rows(self, x, ids):
        self.seen = (self._vectors.shape[0], self._valid_bool[ids].tolist())  # (the protocol's order: grow -> write -> set bits)
        self._vectors[ids] = x
        self._norms[ids] = (x * x).sum(dim=1)

    def _dump_state(self, N):
        return {'vectors': self._vectors[:N].numpy().copy()}

    def _load_state(self, state, N):
        if N:
            self._vectors[:N] = self._to_dev(state['vectors'])
            self._norms[:N] = (self._vectors[:N] ** 2).sum(dim=1)


def _toy(**kw):
    return ToyIndex(4, metric=Metric.EUCLIDEAN, initial_size=64, expand_step_size=64, **kw)


def _rows(ids, salt=0.0):
    ids = np.asarray(ids, dtype=np.float32)
    return np.stack([ids + salt, ids * 2, ids * 0 + 1, -ids], axis=1).astype(np.float32)


def _check_cache(idx):
    assert np.array_equal(idx._valid.numpy().view(np.uint32), _np_pack(idx._valid_bool.numpy()))
    assert idx._valid.numel() == idx.capacity // 32 + (1 if idx.capacity % 32 else 0) + 2  # two spare words


def test_toy_store_life_cycle(tmp_path):
    idx = _toy(ef_construction=9, ef_search=8, max_connection=7)  # (HNSW-only kwargs are dropped)
    assert idx._vectors is None and idx._valid_bool is None and idx.size == 0 and idx.capacity == 64 and idx._n_rows == 0
    idx.delete([1, 2])  # (nothing allocated: nothing happens)
    idx.add_with_ids(np.zeros((0, 4), np.float32), [])
    assert idx.size == 0 and idx._n_rows == 0
    # 1. ids 0..39
    idx.add_with_ids(_rows(range(40)), list(range(40)))
    assert (idx.size, idx.capacity, idx._n_rows) == (40, 64, 40) and idx._vectors.shape == (64, 4) and idx._norms.shape == (64,)
    assert idx._vectors.device.type == idx._valid_bool.device.type == 'cpu'
    _check_cache(idx)
    # 2. id 100: one growth, to ceil(101 / 64) * 64
    idx.add_with_ids(_rows([100]), torch.tensor([100]))
    assert idx.seen == (128, [False])
    assert (idx.size, idx.capacity, idx._n_rows) == (41, 128, 101) and idx._vectors.shape == (128, 4)
    assert not idx._valid_bool[40:100].any() and idx._valid_bool[:40].all() and idx._valid_bool[100] and not idx._valid_bool[101:].any()
    assert np.array_equal(idx._vectors[:40].numpy(), _rows(range(40))) and np.array_equal(idx._vectors[100].numpy(), _rows([100])[0])
    _check_cache(idx)
    # 3. overwrite 31, 32
    idx.update_with_ids(_rows([31, 32], salt=0.5), np.array([31, 32]))
    assert idx.seen == (128, [True, True])
    assert (idx.size, idx._n_rows) == (41, 101)
    assert np.array_equal(idx._vectors[31:33].numpy(), _rows([31, 32], salt=0.5))
    assert np.array_equal(idx._norms[31:33].numpy(), (_rows([31, 32], salt=0.5) ** 2).sum(1))
    assert np.array_equal(idx._vectors[30].numpy(), _rows([30])[0])
    _check_cache(idx)
    # 6. (before the deletes) a filter = selection AND validity, straddling words
    want = np.zeros(idx._valid_bool.numel(), bool)
    want[[5, 31, 32, 100]] = True  # (64: selected, never written)
    for sel in ([5, 31, 32, 64, 100], np.array([5, 31, 32, 64, 100]), torch.tensor([5, 31, 32, 64, 100])):
        assert np.array_equal(idx._filter_bits(sel).numpy().view(np.uint32), _np_pack(want))
    # 4. delete: 63 was never valid
    idx.delete([31, 32, 63, 100])
    assert (idx.size, idx.capacity, idx._n_rows) == (38, 128, 101)
    assert not idx._valid_bool[[31, 32, 63, 100]].any() and int(idx._valid_bool.sum()) == 38
    _check_cache(idx)
    want[[31, 32, 100]] = False
    assert np.array_equal(idx._filter_bits([5, 31, 32, 64, 100]).numpy().view(np.uint32), _np_pack(want))
    # 7. a negative id raises and writes nothing
    before = idx._vectors.clone()
    with pytest.raises(AssertionError):
        idx.add_with_ids(_rows([1, 2]), [3, -1])
    assert torch.equal(idx._vectors, before) and idx.size == 38
    with pytest.raises(AssertionError):
        idx.add_with_ids(_rows([1, 2]), [3])  # (one id per row)
    # 9. dump -> load into a fresh object with a larger and a smaller capacity of its own
    p = tmp_path / 'toy.npy'
    idx.dump(p)
    for own, cap in ((64, 128), (256, 256)):
        other = ToyIndex(4, metric=Metric.EUCLIDEAN, initial_size=own, expand_step_size=64)
        other.load(p)
        assert (other.size, other.capacity, other._n_rows) == (38, cap, 101)
        assert torch.equal(other._vectors[:101], idx._vectors[:101]) and torch.equal(other._norms[:101], idx._norms[:101])
        assert torch.equal(other._valid_bool[:128], idx._valid_bool[:128]) and not other._valid_bool[128:].any()
        _check_cache(other)
    with pytest.raises(AssertionError):
        ToyIndex(5, metric=Metric.EUCLIDEAN).load(p)
    with pytest.raises(AssertionError):
        ToyIndex(4, metric=Metric.COSINE).load(p)
    # 8. reset
    idx.reset()
    assert idx._vectors is None and idx._norms is None and idx._valid_bool is None
    assert (idx.size, idx.capacity, idx._n_rows) == (0, 64, 0)
    idx.add_with_ids(_rows([2]), [2])
    assert (idx.size, idx.capacity, idx._n_rows) == (1, 64, 3)
    _check_cache(idx)


def test_toy_store_loads_a_file_with_the_keys_of_the_first_format(tmp_path):
    """exactly what ``FlatGpuIndex.dump`` wrote before the row store existed: these eight keys, this format string"""
    vec = _rows(range(70))
    valid = np.ones(70, bool)
    valid[[3, 64]] = False
    state = {'format': 'annlite_amd.FlatGpuIndex/1', 'dim': 4, 'metric': int(Metric.EUCLIDEAN), 'n_rows': 70, 'size': 68,
             'capacity': 128, 'vectors': vec, 'valid': valid}
    p = tmp_path / 'old.npy'
    with open(p, 'wb') as f:
        np.save(f, np.array([state], dtype=object), allow_pickle=True)
    idx = _toy()
    idx.load(p)
    assert (idx.size, idx.capacity, idx._n_rows) == (68, 128, 70)
    assert np.array_equal(idx._vectors[:70].numpy(), vec) and np.array_equal(idx._valid_bool[:70].numpy(), valid)
    assert not idx._valid_bool[70:].any()
    # ... and what the store writes has the same keys
    q = tmp_path / 'new.npy'
    idx.dump(q)
    again = np.load(q, allow_pickle=True)[0]
    assert set(again) == set(state) and again['format'] == state['format']
    assert all(np.array_equal(again[key], state[key]) for key in state)


def test_pre_and_the_one_query_search():
    idx = _toy()
    with pytest.raises(AssertionError, match='the query embedding dimension does not match with index dimension: 5 vs 4'):
        idx._pre(np.zeros((2, 5), np.float32))
    with pytest.raises(AssertionError, match='the query embedding dimension does not match with index dimension: 3 vs 4'):
        idx._pre(torch.zeros(3))
    assert idx._pre(np.arange(4.0)).shape == (1, 4) and idx._pre(np.arange(4.0)).dtype == torch.float32
    idx.ready = False
    with pytest.raises(RuntimeError, match='not ready'):  # the readiness hook runs before the dimension check
        idx._pre(np.zeros((2, 5), np.float32))
    # host buffers of a COSINE index are normalised on the host, in the reference's expression
    from annlite_amd.math import l2_normalize_host

    cos = ToyIndex(4, metric=Metric.COSINE)
    x = np.random.RandomState(1).rand(3, 4).astype(np.float32)
    assert np.array_equal(cos._pre(x).numpy(), l2_normalize_host(x))
    # search(): valid entries only, `limit` clipped to the filter's length
    calls = []

    def search_batch(x, limit=10, indices=None):
        calls.append((limit, indices))
        d, i = empty_answer(1, limit, 'cpu')
        d[0, :2], i[0, :2] = torch.tensor([0.5, 1.5]), torch.tensor([9, 4])
        return like_input(isinstance(x, np.ndarray), d, i)

    idx.search_batch = search_batch
    for x in (np.zeros(4, np.float32), torch.zeros(4)):
        d, i = idx.search(x, limit=5)
        assert isinstance(d, np.ndarray) and d.tolist() == [0.5, 1.5] and i.tolist() == [9, 4]
    idx.search(np.zeros(4, np.float32), limit=5, indices=[1, 2, 3])
    assert calls[-1] == (3, [1, 2, 3])
    n = len(calls)
    d, i = idx.search(np.zeros(4, np.float32), limit=5, indices=[])
    assert d.shape == i.shape == (0,) and d.dtype == np.float32 and i.dtype == np.int64 and len(calls) == n
