"""``RowStoreIndex`` -- what every single-device index here shares: rows addressed by offset in lazily allocated device columns,
a validity flag per row, the mutation protocol of ``add_with_ids`` / ``delete``, the reference's one-query ``search`` and the
``np.save`` envelope of ``dump`` / ``load``.  ``FlatGpuIndex`` (vectors + norms; through it ``IvfFlatGpuIndex``) and ``PQFlatGpuIndex``
(codes, optional vectors; through it ``IvfPQGpuIndex`` and ``HnswPQGpuIndex``) declare their columns and write them; how they search
is their own.

Above the class: the pure-torch pieces of a search result that the indexes (and ``multi_gpu.merge_lists_sorted``) put together the
same way -- the empty answer, padding to ``k``, ids taken by position, and the integer key that orders floats like numpy's sort.
"""
import math
from pathlib import Path
from typing import Dict, List, Optional, Tuple, Union

import numpy as np
import torch

from ... import ops
from ...columns import RowMask
from ...enums import Metric
from ...math import l2_normalize_host
from .base import BaseIndex, drop_hnsw_kwargs


# ---------------------------------------------------------------------- result pieces (pure torch, any device)
def empty_answer(B: int, k: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(+inf f32 [B, k], -1 i64 [B, k])``: what an empty index, an empty batch and every missing place answer."""
    return (torch.full((B, k), float('inf'), dtype=torch.float32, device=device),
            torch.full((B, k), -1, dtype=torch.int64, device=device))


def pad_to_k(d: torch.Tensor, i: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``[B, kk <= k]`` lists -> ``[B, k]``, the missing places ``(+inf, -1)``."""
    B, kk = d.shape
    if kk >= k:
        return d, i
    return (torch.cat([d, torch.full((B, k - kk), float('inf'), dtype=d.dtype, device=d.device)], dim=1),
            torch.cat([i, torch.full((B, k - kk), -1, dtype=i.dtype, device=i.device)], dim=1))


def take_by_position(ids: torch.Tensor, pos: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """``ids[b, pos[b, j]]``, -1 where the top-k had no entry (``pos < 0``) or only an infinite distance to offer."""
    i = torch.gather(ids, 1, pos.clamp(min=0))
    return torch.where((pos < 0) | torch.isinf(d), torch.full_like(i, -1), i)


def ranked_answer(ids: torch.Tensor, d: torch.Tensor, pos: torch.Tensor, k: int, sqrt: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """The epilogue of a top-k by position over candidate lists: ids by position, the metric's ``sqrt`` (hnsw/index.py:164-165),
    ``k`` columns."""
    i = take_by_position(ids, pos, d)
    return pad_to_k(torch.sqrt(d) if sqrt else d, i, k)


def _flip(bits: torch.Tensor) -> torch.Tensor:
    return bits ^ ((bits >> 31) & 0x7FFFFFFF)  # (its own inverse: the sign bit stays, the other 31 flip under it)


def float_order_key(dist: torch.Tensor) -> torch.Tensor:
    """f32 -> i64 in int32 range, the signed-comparable image of the float order: -inf < ... < -0.0 < +0.0 < ... < +inf < NaN,
    every NaN the ONE canonical positive NaN (numpy sorts NaN last).  ``(key << 32) | row`` is unique per row, so the smallest such
    keys ARE the (distance, row) order."""
    dist = torch.where(torch.isnan(dist), torch.full_like(dist, float('nan')), dist)
    return _flip(dist.view(torch.int32)).to(torch.int64)


def float_from_key(key: torch.Tensor) -> torch.Tensor:
    """Inverse of ``float_order_key``: the float's own bits back (the canonical NaN for a NaN)."""
    return _flip(key.to(torch.int32)).view(torch.float32)


def like_input(is_np: bool, d: torch.Tensor, i: torch.Tensor):
    """numpy in gives numpy out, device tensors stay on the device."""
    return (d.cpu().numpy(), i.cpu().numpy()) if is_np else (d, i)


# ---------------------------------------------------------------------- a filter per query: the grouping (pure, host)
def group_filters(filters, n_queries: int):
    """One filter per query -> ``(distinct, group_of)``: the distinct filters in the order they first appear -- equal ones (by ``==``)
    are one group; ``{}`` and None are both "no filter", kept as None -- and i64 [B], the group of every query.  ``filters`` must
    be a list or tuple of ``n_queries`` dicts / None, else ``ValueError``."""
    if len(filters) != n_queries:
        raise ValueError(f'filter is a list of {len(filters)} entries for {n_queries} queries: one filter per query')
    distinct, group_of = [], np.empty((n_queries,), dtype=np.int64)
    for b, flt in enumerate(filters):
        if flt is not None and not isinstance(flt, dict):
            raise ValueError(f'filter[{b}] is a {type(flt).__name__}: a dict, {{}} or None per query')
        flt = flt or None
        for g, have in enumerate(distinct):
            if have == flt:
                break
        else:
            g = len(distinct)
            distinct.append(flt)
        group_of[b] = g
    return distinct, group_of


def group_chunks(group_of: np.ndarray, max_groups: int):
    """The launches of a grouped search that takes at most ``max_groups`` bitmaps at a time: ``[(groups, queries, local), ...]`` --
    the ascending ids of up to ``max_groups`` groups THAT HAVE QUERIES, the ascending positions of their queries (None: every query,
    where one launch takes them all) and those queries' group as an index into ``groups``."""
    used = np.unique(group_of)
    if used.size <= max_groups:
        return [(used, None, np.searchsorted(used, group_of))]
    out = []
    for c0 in range(0, used.size, max_groups):
        groups = used[c0:c0 + max_groups]
        queries = np.nonzero(np.isin(group_of, groups))[0]
        out.append((groups, queries, np.searchsorted(groups, group_of[queries])))
    return out


# ---------------------------------------------------------------------- the row store
class RowStoreIndex(BaseIndex):
    FORMAT: str = ''                  # the `format` string of the index's files
    STATE_KEYS: Tuple[str, ...] = ()  # attributes written as integers by `dump` that `load` requires to be the index's own
    ALSO_LOADS: Tuple[str, ...] = ()  # formats of other indexes whose files `load` takes as well (same keys, a subset of the state)

    def __init__(self, dim: int, dtype: np.dtype = np.float32, metric: Metric = Metric.COSINE, **kwargs):
        # HNSW-only kwargs the reference forwards are accepted and ignored
        drop_hnsw_kwargs(kwargs)
        super().__init__(dim, dtype=dtype, metric=metric, **kwargs)
        # device storage is allocated on first use: constructing an index (and the host-side error paths, e.g. "not trained")
        # needs no GPU
        self._drop_storage()
        self.last_filter_batch = None  # 'grouped' / 'looped': how the last search_batch_grouped answered; None: none yet

    # ------------------------------------------------------------------ what a subclass provides
    def _columns(self) -> Dict[str, Optional[Tuple[tuple, torch.dtype]]]:
        """attribute name -> (trailing shape, dtype) of a ``[capacity, ...]`` device column; None: not kept (the attribute is None)"""
        raise NotImplementedError

    def _write_rows(self, x: torch.Tensor, ids: torch.Tensor):
        """store the pre-processed ``x`` [n, D] at the rows ``ids`` i64 [n] (they exist: the store has grown already)"""
        raise NotImplementedError

    def _dump_state(self, N: int) -> dict:
        """the index's own keys of the file: its first ``N`` rows"""
        raise NotImplementedError

    def _load_state(self, state: dict, N: int):
        raise NotImplementedError

    def _check_ready(self):
        """raise if the index cannot take vectors yet (first thing ``_pre`` does)"""

    def _device(self) -> torch.device:
        return ops.device()

    def _to_dev(self, a, dtype=None) -> torch.Tensor:
        return ops.to_dev(a, dtype, dev=self._device())

    def _ids_to_dev(self, ids) -> torch.Tensor:
        if not isinstance(ids, (torch.Tensor, np.ndarray)):
            ids = list(ids)
        return self._to_dev(ids if isinstance(ids, torch.Tensor) else np.asarray(ids, dtype=np.int64), torch.int64)

    # ------------------------------------------------------------------ storage
    def _drop_storage(self):
        for name in self._columns():
            setattr(self, name, None)
        self._valid_bool = None
        self._valid_bits_cache = None
        self._n_rows = 0  # search range = highest written row id + 1

    def _alloc(self, capacity: int):
        dev = self._device()
        for name, spec in self._columns().items():
            setattr(self, name, None if spec is None else torch.zeros((capacity, *spec[0]), dtype=spec[1], device=dev))
        # validity: bool per row is the source of truth (two spare words), the bitmap the kernels read is packed lazily
        self._valid_bool = torch.zeros((((capacity + 31) // 32 + 2) * 32,), dtype=torch.bool, device=dev)
        self._valid_bits_cache = None
        self._capacity = capacity
        self._n_rows = 0
        self._size = 0

    def _ensure_alloc(self):
        if self._valid_bool is None:
            self._alloc(self._capacity)

    def _expand_capacity(self, new_capacity: int):
        self._ensure_alloc()
        old = {name: getattr(self, name) for name in self._columns()}
        old_valid, n, n_rows, size = self._valid_bool, self._capacity, self._n_rows, self._size
        self._alloc(new_capacity)
        for name, col in old.items():
            if col is not None:
                getattr(self, name)[: col.shape[0]] = col
        self._valid_bool[:n] = old_valid[:n]
        self._n_rows, self._size = n_rows, size

    def reset(self, capacity: Optional[int] = None):
        super().reset(capacity=capacity)
        self._drop_storage()

    # ------------------------------------------------------------------ validity
    @staticmethod
    def _pack_bits(flags: torch.Tensor) -> torch.Tensor:
        """bool [32*W] -> int32 [W] bitmap words (bit i of word w = flags[32*w + i]); plumbing only."""
        shifts = torch.arange(32, device=flags.device, dtype=torch.int64)
        packed = (flags.reshape(-1, 32).to(torch.int64) << shifts[None, :]).sum(dim=1)
        return torch.where(packed >= 2 ** 31, packed - 2 ** 32, packed).to(torch.int32)

    @staticmethod
    def _unpack_bits(words: torch.Tensor, n: int) -> torch.Tensor:
        """int32 [W] bitmap words -> bool [n], the first ``n`` flags"""
        shifts = torch.arange(32, device=words.device, dtype=torch.int64)
        return (((words.to(torch.int64) & 0xFFFFFFFF)[:, None] >> shifts[None, :]) & 1).bool().reshape(-1)[:n]

    @property
    def _valid(self) -> torch.Tensor:
        if self._valid_bits_cache is None:
            self._valid_bits_cache = self._pack_bits(self._valid_bool)
        return self._valid_bits_cache

    def _set_bits(self, ids: torch.Tensor, value: bool):
        self._valid_bool[ids] = value
        self._valid_bits_cache = None

    def _filter_bits(self, indices) -> torch.Tensor:
        """`indices` argument of search (flat_index.py:24-27, pq_index.py:42-44, container.py:107-120): restrict to a subset.
        Offsets, or a ``RowMask`` (a filter evaluated on the device, columns.py): its words are the subset already."""
        if isinstance(indices, RowMask):
            return indices.words_for(self._valid.numel()) & self._valid
        sel = torch.zeros_like(self._valid_bool)
        sel[self._ids_to_dev(indices)] = True
        return self._pack_bits(sel & self._valid_bool)

    # ------------------------------------------------------------------ pre-processing (hnsw/index.py:20-48)
    def _pre(self, x) -> torch.Tensor:
        self._check_ready()
        if isinstance(x, np.ndarray) and self.metric == Metric.COSINE:
            # host buffers are normalised with the reference's own numpy expression before the upload (bit-equal vectors =>
            # bit-equal codes / tables / ids); device tensors by the kernel
            xh = np.ascontiguousarray(x.reshape(1, -1) if x.ndim == 1 else x, dtype=np.float32)
            assert xh.shape[-1] == self.dim, (
                f'the query embedding dimension does not match with index dimension: {xh.shape[-1]} vs {self.dim}')
            return self._to_dev(l2_normalize_host(xh), torch.float32)
        x = self._to_dev(x, torch.float32)
        if x.ndim == 1:
            x = x.reshape(1, -1)
        assert x.shape[-1] == self.dim, (
            f'the query embedding dimension does not match with index dimension: {x.shape[-1]} vs {self.dim}')
        if self.metric == Metric.COSINE:
            x = ops.l2_normalize(x)
        return x

    # ------------------------------------------------------------------ mutation
    def add_with_ids(self, x, ids: List[int], **kwargs):
        """Two host round trips: the ids' range (which may grow the store) and the count of rows that were not valid before."""
        x = self._pre(x)
        self._ensure_alloc()
        ids_t = self._ids_to_dev(ids)
        assert ids_t.numel() == x.shape[0]
        if ids_t.numel() == 0:
            return
        min_id, max_id = torch.stack(torch.aminmax(ids_t)).tolist()
        assert min_id >= 0  # (a negative id would address a row outside the columns)
        max_id += 1
        if max_id > self.capacity:
            steps = math.ceil(max_id / self.expand_step_size)  # hnsw/index.py:132-135
            self._expand_capacity(steps * self.expand_step_size)
        self._write_rows(x, ids_t)
        was_valid = self._valid_bool[ids_t]
        self._set_bits(ids_t, True)
        self._size += int((~was_valid).sum().item())
        self._n_rows = max(self._n_rows, max_id)

    def update_with_ids(self, x, ids: List[int], **kwargs):
        """flat_index.py:70-71 semantics (overwrite rows)."""
        self.add_with_ids(x, ids)

    def delete(self, ids: List[int]):
        if self._valid_bool is None or len(ids) == 0:
            return
        ids_t = self._ids_to_dev(ids)
        was_valid = self._valid_bool[ids_t]
        self._set_bits(ids_t, False)
        self._size -= int(was_valid.sum().item())

    # ------------------------------------------------------------------ search
    def search_batch(self, x, limit: int = 10, indices=None):
        raise NotImplementedError

    MAX_FILTER_GROUPS = 64  # bitmaps per grouped launch (FlatGpuIndex): 64 masks are 8 MB at 1M rows, 80 MB at 10M

    @staticmethod
    def _check_groups(n_queries: int, selections, group_of) -> np.ndarray:
        """``group_of`` as i64 [B] on the host, every entry in ``[0, len(selections))``, else ``ValueError``"""
        g = np.asarray(group_of.cpu() if isinstance(group_of, torch.Tensor) else group_of, dtype=np.int64).reshape(-1)
        if g.size != n_queries:
            raise ValueError(f'group_of has {g.size} entries for {n_queries} queries')
        if g.size and (int(g.min()) < 0 or int(g.max()) >= len(selections)):
            raise ValueError(f'group_of must lie in [0, {len(selections)})')
        return g

    def search_batch_grouped(self, x, limit: int = 10, selections=(), group_of=()):
        """A filter per query ("a filter per query"): ``selections`` is a sequence of G values, each anything
        ``search_batch(indices=...)`` takes -- offsets, a ``RowMask``, None for no filter --, and query b is searched under
        ``selections[group_of[b]]``.  ``(dists [B, limit], ids [B, limit])`` as ``search_batch`` returns them, every row what
        ``search_batch`` answers that query under its selection, padded with (+inf, -1).

        This is the form every index has: one ``search_batch`` per group that has queries (``last_filter_batch = 'looped'``), so a
        pruned or graph search stays the search it is per group.  ``FlatGpuIndex`` answers ``limit <= 64`` in one launch."""
        is_np = not isinstance(x, torch.Tensor)
        xs = x.reshape(1, -1) if x.ndim == 1 else x
        B, k = xs.shape[0], int(limit)
        assert k >= 1
        group = self._check_groups(B, selections, group_of)
        self.last_filter_batch = 'looped'
        out = None
        for g in np.unique(group):
            idx = np.nonzero(group == g)[0]
            sel = selections[int(g)]
            if sel is not None and len(sel) == 0:
                continue  # (no rows: the padding is the answer)
            gd, gi = self.search_batch(xs[idx if is_np else torch.as_tensor(idx, device=xs.device)], limit=k, indices=sel)
            gd, gi = pad_to_k(torch.as_tensor(gd), torch.as_tensor(gi), k)
            if out is None:
                out = empty_answer(B, k, gd.device)
            at = torch.as_tensor(idx, device=gd.device)
            out[0][at], out[1][at] = gd[:, :k], gi[:, :k]
        if out is None:
            out = empty_answer(B, k, torch.device('cpu') if is_np else self._device())
        return (out[0].numpy(), out[1].numpy()) if is_np else out

    def search(self, x, limit: int = 10, indices=None):
        """ONE query, reference signature (hnsw/index.py:139-167): ``(dists[k'], ids[k'])`` numpy, ``k' <= limit`` valid entries
        only."""
        if indices is not None and len(indices) < limit:
            limit = len(indices)  # hnsw/index.py:153-154
        if limit <= 0:
            return np.empty((0,), np.float32), np.empty((0,), np.int64)
        d, i = self.search_batch(x, limit=limit, indices=indices)
        if isinstance(d, torch.Tensor):
            d, i = d.cpu().numpy(), i.cpu().numpy()
        d, i = d[0], i[0]
        keep = i >= 0
        return d[keep], i[keep]

    # ------------------------------------------------------------------ persistence (own format): one object dict in one np.save
    def dump(self, index_file: Union[str, Path]):
        """hnsw/index.py:121-122 analogue: the first ``_n_rows`` rows and their validity."""
        self._ensure_alloc()
        N = self._n_rows
        state = {'format': self.FORMAT, **{key: int(getattr(self, key)) for key in self.STATE_KEYS},
                 'n_rows': N, 'size': self._size, 'capacity': self._capacity,
                 'valid': self._valid_bool[:N].cpu().numpy(), **self._dump_state(N)}
        with open(str(index_file), 'wb') as f:
            np.save(f, np.array([state], dtype=object), allow_pickle=True)

    def load(self, index_file: Union[str, Path]):
        with open(str(index_file), 'rb') as f:
            state = np.load(f, allow_pickle=True)[0]
        assert state['format'] == self.FORMAT or state['format'] in self.ALSO_LOADS
        assert all(state[key] == getattr(self, key) for key in self.STATE_KEYS)
        self._alloc(max(int(state['capacity']), self._capacity))
        N = int(state['n_rows'])
        self._load_state(state, N)
        v = self._to_dev(state['valid'])
        self._valid_bool[: v.numel()] = v
        self._valid_bits_cache = None
        self._n_rows, self._size = N, int(state['size'])
