"""``FlatGpuIndex`` -- exact search over un-quantised float32 vectors on one MI355X: what the reference builds for
``AnnLite(n_dim)`` without ``n_subvectors`` (``HnswIndex`` on float vectors, annlite/core/index/hnsw/index.py:139-167; brute-force
form ``FlatIndex``, annlite/core/index/flat_index.py:15-39: ``cdist`` + ``top_k``).

Same plug-in surface as ``PQFlatGpuIndex`` (``add_with_ids`` / ``update_with_ids`` / ``delete`` / ``reset`` / ``search`` /
``search_batch`` / ``dump`` / ``load``, capacity growing by ``expand_step_size``, device storage allocated on first use).  HBM
holds ``f32 [capacity, D]`` vectors, ``f32 [capacity]`` squared norms (written by a kernel at add / update) and the validity
bitmap.  A search is ONE C call (``annlite_flat_search_topk``): an f32 MFMA contraction filters the table
against a per-query bound with a proven slack, a wave per query re-scores the rows that passed in ``annlite_rerank_topk``'s
arithmetic.  The answer is exact in that arithmetic: a stored vector searched with itself comes back at distance 0.0.

Where it is slow (and still exact): the filter's slack is relative to ``|x|^2 + |q|^2``, not to the distance.  Data with a large
common offset (every coordinate near 1000) makes it exceed every distance: all rows pass, the lists overflow and each query is
answered by one wave over ALL rows (``last_overflowed`` counts them) -- centre such data before indexing it.  The same route serves
NaN / infinite queries and searches restricted (``indices=``, deletes) to fewer than about k rows in 4096.
"""
import math
from pathlib import Path
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from ... import ops
from ...enums import Metric
from ...math import l2_normalize_host
from .base import BaseIndex


def flat_slack_constants(metric: Metric, dim: int) -> Tuple[np.float32, np.float32]:
    """``(c_rel, c_abs)`` of the filter's slack ``c_rel * fl(|x|^2 + |q|^2) + c_abs`` -- the numbers the library hands its filter
    kernel (``annlite_flat_slack``; derivation: DESIGN.md section 3.6)."""
    return ops.flat_slack(int(Metric(metric)), dim)


class FlatGpuIndex(BaseIndex):
    def __init__(self, dim: int, dtype: np.dtype = np.float32, metric: Metric = Metric.COSINE,
                 index_file: Optional[Union[str, Path]] = None, **kwargs):
        # HNSW-only kwargs the reference forwards (ef_construction, ef_search, max_connection) are accepted and ignored: the
        # search is exhaustive and exact
        for k in ('ef_construction', 'ef_search', 'max_connection'):
            kwargs.pop(k, None)
        super().__init__(dim, dtype=dtype, metric=metric, **kwargs)
        self._ws = ops.ScanWorkspace()
        # device storage is allocated on first use: constructing an index needs no GPU
        self._vectors = None
        self._norms = None
        self._valid_bool = None
        self._valid_bits_cache = None
        self._n_rows = 0
        self._overflowed = 0  # (of the last search_batch; None: ask the library's workspace)
        if index_file:
            self.load(index_file)

    # ------------------------------------------------------------------ storage
    def _alloc(self, capacity: int):
        dev = ops.device()
        self._vectors = torch.zeros((capacity, self.dim), dtype=torch.float32, device=dev)
        self._norms = torch.zeros((capacity,), dtype=torch.float32, device=dev)
        self._valid_bool = torch.zeros((((capacity + 31) // 32 + 2) * 32,), dtype=torch.bool, device=dev)
        self._valid_bits_cache = None
        self._capacity = capacity
        self._n_rows = 0  # search range = highest written row id + 1
        self._size = 0

    def _ensure_alloc(self):
        if self._vectors is None:
            self._alloc(self._capacity)

    def _expand_capacity(self, new_capacity: int):
        self._ensure_alloc()
        old_vec, old_norms, old_valid, n_rows, size = self._vectors, self._norms, self._valid_bool, self._n_rows, self._size
        self._alloc(new_capacity)
        n = old_vec.shape[0]
        self._vectors[:n] = old_vec
        self._norms[:n] = old_norms
        self._valid_bool[:n] = old_valid[:n]
        self._n_rows, self._size = n_rows, size

    # ------------------------------------------------------------------ pre-processing (hnsw/index.py:20-48)
    def _pre(self, x) -> torch.Tensor:
        if isinstance(x, np.ndarray) and self.metric == Metric.COSINE:
            # host buffers are normalised with the reference's own numpy expression before the upload; device tensors by the kernel
            xh = np.ascontiguousarray(x.reshape(1, -1) if x.ndim == 1 else x, dtype=np.float32)
            assert xh.shape[-1] == self.dim, (
                f'the query embedding dimension does not match with index dimension: {xh.shape[-1]} vs {self.dim}')
            return ops.to_dev(l2_normalize_host(xh), torch.float32)
        x = ops.to_dev(x, torch.float32)
        if x.ndim == 1:
            x = x.reshape(1, -1)
        assert x.shape[-1] == self.dim, (
            f'the query embedding dimension does not match with index dimension: {x.shape[-1]} vs {self.dim}')
        if self.metric == Metric.COSINE:
            x = ops.l2_normalize(x)
        return x

    @staticmethod
    def _pack_bits(flags: torch.Tensor) -> torch.Tensor:
        """bool [32*W] -> int32 [W] bitmap words (bit i of word w = flags[32*w + i]); plumbing only."""
        shifts = torch.arange(32, device=flags.device, dtype=torch.int64)
        packed = (flags.reshape(-1, 32).to(torch.int64) << shifts[None, :]).sum(dim=1)
        return torch.where(packed >= 2 ** 31, packed - 2 ** 32, packed).to(torch.int32)

    @property
    def _valid(self) -> torch.Tensor:
        if self._valid_bits_cache is None:
            self._valid_bits_cache = self._pack_bits(self._valid_bool)
        return self._valid_bits_cache

    def _set_bits(self, ids: torch.Tensor, value: bool):
        self._valid_bool[ids] = value
        self._valid_bits_cache = None

    # ------------------------------------------------------------------ mutation
    def add_with_ids(self, x, ids: List[int], **kwargs):
        x = self._pre(x)
        self._ensure_alloc()
        ids_t = ops.to_dev(np.asarray(ids, dtype=np.int64) if not isinstance(ids, torch.Tensor) else ids, torch.int64)
        assert ids_t.numel() == x.shape[0]
        if ids_t.numel() == 0:
            return
        assert int(ids_t.min().item()) >= 0
        max_id = int(ids_t.max().item()) + 1
        if max_id > self.capacity:
            steps = math.ceil(max_id / self.expand_step_size)  # hnsw/index.py:132-135
            self._expand_capacity(steps * self.expand_step_size)
        self._vectors[ids_t] = x  # flat_index.py:41-50 `_data[ids] = x`
        ops.flat_row_norms(self._vectors, ids=ids_t, out=self._norms)
        was_valid = self._valid_bool[ids_t]
        self._set_bits(ids_t, True)
        self._size += int((~was_valid).sum().item())
        self._n_rows = max(self._n_rows, max_id)

    def update_with_ids(self, x, ids: List[int], **kwargs):
        """flat_index.py:70-71 semantics (overwrite rows)."""
        self.add_with_ids(x, ids)

    def delete(self, ids: List[int]):
        if self._vectors is None or len(ids) == 0:
            return
        ids_t = ops.to_dev(np.asarray(list(ids), dtype=np.int64), torch.int64)
        was_valid = self._valid_bool[ids_t]
        self._set_bits(ids_t, False)
        self._size -= int(was_valid.sum().item())

    def reset(self, capacity: Optional[int] = None):
        super().reset(capacity=capacity)
        self._vectors = None
        self._norms = None
        self._valid_bool = None
        self._valid_bits_cache = None
        self._n_rows = 0

    @property
    def size(self):
        return self._size

    # ------------------------------------------------------------------ search
    def _filter_bits(self, indices) -> torch.Tensor:
        """`indices` argument of search (flat_index.py:24-27, container.py:107-120): restrict to a subset."""
        idx = ops.to_dev(np.asarray(indices, dtype=np.int64) if not isinstance(indices, torch.Tensor) else indices, torch.int64)
        sel = torch.zeros_like(self._valid_bool)
        sel[idx] = True
        return self._pack_bits(sel & self._valid_bool)

    @property
    def last_overflowed(self) -> int:
        """Queries of the last ``search_batch`` whose candidate list overflowed: they were answered by exact sums over all rows
        -- the slower route.  0 after a search that ran no filter (empty index, empty batch)."""
        if self._overflowed is None:
            self._overflowed = ops.flat_overflow_count(self._ws)
        return self._overflowed

    def search_batch(self, x, limit: int = 10, indices=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """All queries of ``x`` [B, D] in one call.  ``(dists f32 [B, k], ids i64 [B, k])`` ascending by (distance, id), NaN
        distances last; missing -> (+inf, -1).  numpy in gives numpy out, device tensors stay on the device."""
        is_np = not isinstance(x, torch.Tensor)
        q = self._pre(x)
        B = q.shape[0]
        k = int(limit)
        assert k >= 1
        N = self._n_rows
        dev = q.device
        self._overflowed = 0
        if N == 0 or B == 0:
            d = torch.full((B, k), float('inf'), dtype=torch.float32, device=dev)
            i = torch.full((B, k), -1, dtype=torch.int64, device=dev)
        else:
            valid = self._valid if indices is None else self._filter_bits(indices)
            if k <= 64:
                d, i = ops.flat_search_topk(int(self.metric), q, self._vectors, self._norms, k, valid_bits=valid, n_rows=N,
                                            sqrt=self.metric == Metric.EUCLIDEAN, workspace=self._ws)  # hnsw/index.py:164-165
                self._overflowed = None  # (read from the workspace when asked for: it costs a synchronisation)
            else:
                d, i = self._search_large_k(q, k, valid, N)
        if is_np:
            return d.cpu().numpy(), i.cpu().numpy()
        return d, i

    def _keyed_topk(self, q, cand, ok, kk):
        """The ``kk`` nearest of each query's candidates ``cand`` i64 [b, R] (``ok``: which entries count) by exact distance
        (``annlite_exact_gather_dist``: a wave per pair, the numbers of the k <= 64 path): i64 keys -- order-preserving bits of the
        distance << 32 | row id, unique, so the smallest keys ARE the (distance, id) order, NaN last -- and one ``torch.topk``."""
        dist = ops.exact_gather_dist(int(self.metric), q, self._vectors, cand)
        dist = torch.where(torch.isnan(dist), torch.full_like(dist, float('nan')), dist)  # one NaN, sign bit clear: behind +inf
        bits = dist.view(torch.int32)
        bits = bits ^ ((bits >> 31) & 0x7FFFFFFF)  # signed-comparable image of the float order
        key_none = torch.iinfo(torch.int64).max
        keys = (bits.to(torch.int64) << 32) | cand.clamp(min=0)
        keys = torch.where(ok, keys, torch.full_like(keys, key_none))
        top = torch.topk(keys, kk, dim=1, largest=False, sorted=True).values
        none = top == key_none
        hi = (top >> 32).to(torch.int32)
        sd = (hi ^ ((hi >> 31) & 0x7FFFFFFF)).view(torch.float32)
        sd = torch.where(none, torch.full_like(sd, float('inf')), sd)
        si = torch.where(none | (sd == float('inf')), torch.full_like(top, -1), top & 0xFFFFFFFF)  # (+inf: a missing place, as annlite_rerank_topk)
        return sd, si

    def _all_rows_topk(self, q, kk, vb, N):
        """``_keyed_topk`` over every row, in query chunks: the route of small tables and of overflowed lists."""
        rows = torch.arange(N, device=q.device, dtype=torch.int64)
        chunk = max(1, min(q.shape[0], (1 << 25) // max(N, 1)))
        out = [self._keyed_topk(q[b0:b0 + chunk].contiguous(), rows[None, :].expand(min(chunk, q.shape[0] - b0), N).contiguous(),
                                vb[None, :].expand(min(chunk, q.shape[0] - b0), N), kk) for b0 in range(0, q.shape[0], chunk)]
        return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])

    def _search_large_k(self, q, k, valid, N):
        """k > 64 (beyond the wave-resident lists).  The same filter as the k <= 64 search with ONE bound -- the k-th smallest
        exact distance among every stride-th row, stride = cap / (2 k), so that about cap / 2 rows per query pass -- then exact
        distances and a keyed top-k over the candidate lists.  Queries whose list overflowed, and shapes without room for a sample
        (N <= 2 cap, k > cap / 4), take exact distances over all rows.  Correct, not tuned: the sample's distances are a wave per
        (query, sampled row), N / stride of them per query."""
        dev = q.device
        B = q.shape[0]
        shifts = torch.arange(32, device=dev, dtype=torch.int64)
        vb = (((valid.to(torch.int64) & 0xFFFFFFFF)[:, None] >> shifts[None, :]) & 1).bool().reshape(-1)[:N]
        kk = min(k, N)
        cap = ops.flat_list_capacity()
        stride = cap // (2 * kk)  # rows at or below the k-th of every stride-th row: about k stride +- stride sqrt(k) <= cap / 2 + ...
        if N <= 2 * cap or stride < 2:
            d, i = self._all_rows_topk(q, kk, vb, N)
        else:
            sample = torch.arange(0, N, stride, device=dev, dtype=torch.int64)
            s_ok = vb[sample]
            chunk = max(1, min(B, (1 << 25) // sample.numel()))
            bounds = []
            for b0 in range(0, B, chunk):
                nb = min(chunk, B - b0)
                ds = ops.exact_gather_dist(int(self.metric), q[b0:b0 + nb].contiguous(), self._vectors, sample[None, :].expand(nb, -1).contiguous())
                ds = torch.where(s_ok[None, :], torch.nan_to_num(ds, nan=float('inf'), posinf=float('inf'), neginf=float('-inf')),
                                 torch.full_like(ds, float('inf')))
                bounds.append(torch.topk(ds, kk, dim=1, largest=False).values[:, kk - 1] if sample.numel() >= kk
                              else torch.full((nb,), float('inf'), device=dev))
            bound = torch.cat(bounds).contiguous()  # (+inf -- fewer than k valid sampled rows, NaN distances -- passes everything)
            cand32, count = ops.flat_filter(int(self.metric), q, self._vectors, self._norms, bound, valid_bits=valid, n_rows=N)
            over = count > cap
            ok = torch.arange(cap, device=dev)[None, :] < count[:, None]
            cand = torch.where(ok, cand32.to(torch.int64), torch.full((1, 1), -1, dtype=torch.int64, device=dev))
            chunk = max(1, min(B, (1 << 25) // cap))
            out = [self._keyed_topk(q[b0:b0 + chunk].contiguous(), cand[b0:b0 + chunk].contiguous(), ok[b0:b0 + chunk], kk)
                   for b0 in range(0, B, chunk)]
            d, i = torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])
            over_idx = torch.nonzero(over).reshape(-1)
            self._overflowed = int(over_idx.numel())
            if self._overflowed:
                od, oi = self._all_rows_topk(q[over_idx].contiguous(), kk, vb, N)
                d[over_idx], i[over_idx] = od, oi
        if kk < k:
            d = torch.cat([d, torch.full((d.shape[0], k - kk), float('inf'), device=dev)], dim=1)
            i = torch.cat([i, torch.full((i.shape[0], k - kk), -1, dtype=torch.int64, device=dev)], dim=1)
        if self.metric == Metric.EUCLIDEAN:
            d = torch.sqrt(d)
        return d, i

    def search(self, x, limit: int = 10, indices=None):
        """ONE query, reference signature (hnsw/index.py:139-167): ``(dists[k'], ids[k'])`` numpy, valid entries only."""
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

    # ------------------------------------------------------------------ persistence (own format)
    def dump(self, index_file: Union[str, Path]):
        """hnsw/index.py:121-122 analogue: vectors (as stored: normalised for COSINE) and validity; norms are recomputed on load."""
        self._ensure_alloc()
        N = self._n_rows
        state = {
            'format': 'annlite_amd.FlatGpuIndex/1',
            'dim': self.dim, 'metric': int(self.metric), 'n_rows': N, 'size': self._size, 'capacity': self._capacity,
            'vectors': self._vectors[:N].cpu().numpy(), 'valid': self._valid_bool[:N].cpu().numpy(),
        }
        with open(str(index_file), 'wb') as f:
            np.save(f, np.array([state], dtype=object), allow_pickle=True)

    def load(self, index_file: Union[str, Path]):
        with open(str(index_file), 'rb') as f:
            state = np.load(f, allow_pickle=True)[0]
        assert state['format'] == 'annlite_amd.FlatGpuIndex/1'
        assert state['dim'] == self.dim and state['metric'] == int(self.metric)
        self._alloc(max(int(state['capacity']), self._capacity))
        N = int(state['n_rows'])
        if N:
            self._vectors[:N] = ops.to_dev(state['vectors'])
            ops.flat_row_norms(self._vectors, n=N, out=self._norms)
        v = ops.to_dev(state['valid'])
        self._valid_bool[: v.numel()] = v
        self._valid_bits_cache = None
        self._n_rows, self._size = N, int(state['size'])
