"""``IvfFlatGpuIndex`` -- exact float32 search over coarse cells on one MI355X: the reference's ``AnnLite(n_cells > 1)`` in its
default configuration, without ``n_subvectors`` (``VQCodec`` coarse quantiser annlite/core/codec/vq.py, ``_cell_selection``
annlite/index.py:458-466, one float index per cell + ``CellContainer.ivf_search`` merge, container.py:88-144) as ONE row store and
one C call for all queries and cells.

Semantics:
  * ``n_probe`` ``None`` or ``>= n_cells`` (what the reference always does: ``n_probe = max(n_probe, n_cells)``, index.py:94): every
    cell is visited -- the search IS ``FlatGpuIndex.search_batch``.
  * ``n_probe < n_cells`` (this build's extension, opt-in): the top-k of the live rows whose cell is one of the query's ``n_probe``
    nearest, in ``annlite_rerank_topk``'s arithmetic bit for bit (what ``FlatGpuIndex`` returns for those rows), ascending by
    (distance, row id), NaN last, missing places ``(+inf, -1)``.  The rows that are scanned are answered exactly; what a pruned
    search can miss is a neighbour in a cell it did not probe.

Layout on top of the float index's storage (vectors, norms, validity -- by offset, and NOT copied):
  * ``_cell_of``  i32 [capacity]   cell of every offset (cells.py)
  * ``_cell_cnorms`` f32 [capacity]  ``|fl(x - centroid of x's cell)|^2`` -- only with ``cell_filter='bf16x3'`` and EUCLIDEAN: the norms
    the split filter over cell tiles reads (written at add / update after the cell is assigned; recomputed by ``load``)
  * sealed view, rebuilt lazily after a mutation (one sort over the live rows):
      ``_perm``       i32 [n_live]  the live offsets grouped by cell, ascending inside a cell
      ``_cell_rows``  i64 [C, 2]    (begin, end) of every cell in ``_perm``
      ``_cell_order`` i32 [C]       cells by descending size
      on the host: the cells' lengths in descending order, summed from the largest on (``_sizes_cum``): the largest cell and the
      sum of the P largest are the two numbers the search call wants
"""
from typing import Optional

import numpy as np
import torch

from ... import ops
from ...enums import Metric
from ..codec.vq import VQCodec
from .cells import CellColumnMixin
from .flat_gpu import FlatGpuIndex, is_f16, is_i8
from .row_store import RowStoreIndex, empty_answer, like_input, pad_to_k


class IvfFlatGpuIndex(CellColumnMixin, FlatGpuIndex):
    """
    :param cell_filter: ``'f32'`` (default): the f32 MFMA filter over the (cell, queries) tiles.  ``'bf16x3'``: the split-bf16 filter
        over the same tiles ("split filter over cell tiles") -- the same answer bit for bit, ``dim <= 32768``.
        With EUCLIDEAN every tile is centred on the centroid of its cell, so the slack is relative to the rows' and queries' distances
        to that centroid and does not grow with a common offset of the data; INNER_PRODUCT and COSINE run it uncentred.  The centroids
        are the ``vq_codec``'s codebook as it is at the first ``add_with_ids``, frozen until ``reset()`` (``cell_centres_``).  The
        every-cell search, ``limit > 64`` and searches over at most 4096 probed rows are the same under either value.
    :param flat_filter, centre: the every-cell search's options in ``FlatGpuIndex``; accepted and ignored here (it stays ``'f32'``).
    """
    FORMAT = 'annlite_amd.IvfFlatGpuIndex/1'
    CELL_FILTERS = ('f32', 'bf16x3')
    # (a filter per query: one search_batch per group -- the pruned search stays the search it is under every selection)
    search_batch_grouped = RowStoreIndex.search_batch_grouped

    def __init__(self, dim: int, vq_codec: Optional[VQCodec] = None, n_probe: Optional[int] = None, metric: Metric = Metric.COSINE,
                 cell_filter: str = 'f32', **kwargs):
        assert vq_codec is not None, 'IvfFlatGpuIndex needs a VQCodec'
        if cell_filter not in self.CELL_FILTERS:
            raise ValueError(f"cell_filter={cell_filter!r}: 'f32' (the f32 MFMA filter over the cell tiles) or 'bf16x3' (the split-bf16 "
                             "filter, every tile centred on its cell's centroid)")
        if cell_filter == 'bf16x3' and dim > self.SPLIT_MAX_DIM:
            raise ValueError(f"cell_filter='bf16x3' takes dim <= {self.SPLIT_MAX_DIM}")
        self.vq_codec = vq_codec
        self.n_probe = n_probe  # None: every cell (the reference's behaviour)
        self.cell_filter = cell_filter
        self.last_cell_filter = None  # 'f32' / 'bf16x3': the cell-tile filter of the last search_batch; None: it ran none
        self._cell_centred = cell_filter == 'bf16x3' and Metric(metric) == Metric.EUCLIDEAN
        self._cell_centres_dev = None
        self._stored_cell_centres = None  # (between `_load_state` and the end of `load`: the centres an index file carried)
        self._sealed = False
        self._perm = self._cell_rows = self._cell_order = self._sizes_cum = None
        # (accepted and ignored: this index's every-cell search is the f32 one -- DESIGN.md section 10)
        kwargs.pop('flat_filter', None)
        kwargs.pop('centre', None)
        if is_f16(kwargs.get('dtype', 'float32')):
            raise NotImplementedError('dtype=np.float16: the cell-tile kernels read f32 rows only (half-precision rows exist in the '
                                      'exhaustive FlatGpuIndex: no graph, n_cells=1)')
        if is_i8(kwargs.get('dtype', 'float32')):
            raise NotImplementedError('dtype=np.int8: the cell-tile kernels read f32 rows only (int8 rows exist in the '
                                      'exhaustive FlatGpuIndex: no graph, n_cells=1)')
        super().__init__(dim, metric=metric, **kwargs)

    # ------------------------------------------------------------------ the split filter's centres and its norms column
    @property
    def cell_centres_(self):
        """The centroids the split filter centres its tiles on, f32 ``[n_cells, dim]``; None: none (the f32 filter, another metric, or
        before the first rows arrived)."""
        return None if self._cell_centres_dev is None else self._cell_centres_dev.cpu().numpy()

    def _fix_cell_centres(self, stored=None):
        """Settle the centres once: the ones an index file carried, else the codebook as it is now.  A centre that moved would
        invalidate ``_cell_cnorms``: the snapshot is the index's own until ``reset()``."""
        if not self._cell_centred or self._cell_centres_dev is not None:
            return
        if stored is not None:
            stored = np.asarray(stored, dtype=np.float32)
            assert stored.shape == (self.n_cells, self.dim), f'cell_centres has shape {stored.shape}'
            self._cell_centres_dev = self._to_dev(stored, torch.float32).contiguous()
        else:
            self._cell_centres_dev = self.vq_codec.codebook_dev.to(torch.float32).contiguous().clone()

    def _columns(self):
        """``_cell_cnorms``: ``|fl(x - centroid of x's cell)|^2``, kept only where the split filter has centres (it reads ``_norms``
        otherwise)"""
        return {**super()._columns(), '_cell_cnorms': ((), torch.float32) if self._cell_centred else None}

    def add_with_ids(self, x, ids, **kwargs):
        ids_t = self._ids_to_dev(ids)
        if ids_t.numel() == 0:
            return
        super().add_with_ids(x, ids_t)  # (rows, then their cells)
        if self._cell_centred:  # (after `_cell_of`: a row an update moved gets the norm against its new centroid)
            self._fix_cell_centres()
            ops.ivf_flat_centred_norms(self._vectors, self._cell_centres_dev, self._cell_of, ids=ids_t, out=self._cell_cnorms)

    def reset(self, capacity: Optional[int] = None):
        super().reset(capacity=capacity)
        self._cell_centres_dev = None

    def _dump_state(self, N):
        """``cell_centres`` (optional key): the split filter's"""
        state = super()._dump_state(N)
        if self._cell_centres_dev is not None:
            state['cell_centres'] = self.cell_centres_
        return state

    def _load_state(self, state, N):
        super()._load_state(state, N)
        self._cell_centres_dev = None
        self._stored_cell_centres = state.get('cell_centres')  # (a file without the key -- an older one, an f32 index's: the codebook)

    def load(self, index_file):
        super().load(index_file)  # (rows, then `.cells.npy`)
        stored, self._stored_cell_centres = self._stored_cell_centres, None
        if self._cell_centred and self._n_rows:
            self._fix_cell_centres(stored)
            ops.ivf_flat_centred_norms(self._vectors, self._cell_centres_dev, self._cell_of, n=self._n_rows, out=self._cell_cnorms)

    # ------------------------------------------------------------------ sealed (cell-grouped) view
    def _seal(self):
        if self._sealed:
            return
        N, C = self._n_rows, self.n_cells
        live = torch.nonzero(self._valid_bool[:N]).flatten()  # ascending offsets
        cell = self._cell_of[:N][live].to(torch.int64)
        order = torch.sort(cell, stable=True).indices          # by cell, offsets ascending inside a cell
        self._perm = live[order].to(torch.int32).contiguous()
        counts = torch.bincount(cell, minlength=C)
        end = torch.cumsum(counts, 0)
        self._cell_rows = torch.stack([end - counts, end], dim=1).contiguous()
        by_size = torch.sort(counts, descending=True, stable=True)
        self._cell_order = by_size.indices.to(torch.int32).contiguous()
        self._sizes_cum = torch.cumsum(by_size.values, 0).cpu().numpy()  # (the seal's one host read)
        self._sealed = True

    # ------------------------------------------------------------------ search
    def search_batch(self, x, limit: int = 10, indices=None, n_probe: Optional[int] = None, filter_route: Optional[str] = None):
        """``FlatGpuIndex.search_batch`` over the rows of each query's ``n_probe`` nearest cells (every cell: that search itself, with
        its ``filter_route``; the pruned search scans cell tiles under the bitmap whatever the route, and reports ``'mask'``)."""
        P = self.n_probe if n_probe is None else n_probe
        C = self.n_cells
        self.last_cell_filter = None
        if P is None or P >= C:
            return super().search_batch(x, limit=limit, indices=indices, filter_route=filter_route)
        self.last_filter_route = 'mask'
        is_np = not isinstance(x, torch.Tensor)
        q = self._pre(x)
        B, k = q.shape[0], int(limit)
        assert k >= 1
        P = max(1, int(P))
        self._overflowed = 0
        if self._n_rows == 0 or B == 0 or self._size == 0:
            d, i = empty_answer(B, k, q.device)
        else:
            self._seal()
            valid = self._valid if indices is None else self._filter_bits(indices)
            cells = self.probe_cells(q, P)
            max_cell, max_probed = int(self._sizes_cum[0]), int(self._sizes_cum[P - 1])
            if k <= 64 and self.cell_filter == 'bf16x3':
                d, i = ops.ivf_flat_search_topk_split(int(self.metric), q, self._vectors,
                                                      self._cell_cnorms if self._cell_centred else self._norms, cells, C, self._perm,
                                                      self._cell_rows, self._cell_order, max_cell, max_probed, k,
                                                      centres=self._cell_centres_dev if self._cell_centred else None,
                                                      cell_of=self._cell_of if self._cell_centred else None, valid_bits=valid,
                                                      n_rows=self._n_rows, sqrt=self.metric == Metric.EUCLIDEAN, workspace=self._ws)
                self._overflowed = None
                self.last_cell_filter = 'bf16x3' if max_probed >= self.FILTER_MIN_ROWS else None
            elif k <= 64:
                d, i = ops.ivf_flat_search_topk(int(self.metric), q, self._vectors, self._norms, cells, C, self._perm, self._cell_rows,
                                                self._cell_order, max_cell, max_probed, k, valid_bits=valid, n_rows=self._n_rows,
                                                sqrt=self.metric == Metric.EUCLIDEAN, workspace=self._ws)  # hnsw/index.py:164-165
                self._overflowed = None  # (read from the workspace when asked for: it costs a synchronisation)
                self.last_cell_filter = 'f32' if max_probed >= self.FILTER_MIN_ROWS else None
            else:
                d, i = self._search_large_k_cells(q, k, valid, cells, max_probed)
        return like_input(is_np, d, i)

    def _probed_rows(self, cells: torch.Tensor, R: int):
        """``(cand i64 [b, R], ok bool [b, R])``: every query's probed rows as one dense block -- the ranges of its cells in
        ``_perm`` back to back, -1 behind them."""
        rng = self._cell_rows[cells.to(torch.int64)]                # [b, P, 2]
        cum = torch.cumsum(rng[:, :, 1] - rng[:, :, 0], dim=1)      # [b, P] rows up to and including probe p
        j = torch.arange(R, device=cells.device, dtype=torch.int64)[None, :].expand(cells.shape[0], R).contiguous()
        p = torch.searchsorted(cum, j, right=True)                  # probe that position j falls into (P: behind the last row)
        ok = p < cells.shape[1]
        p = p.clamp(max=cells.shape[1] - 1)
        first = torch.gather(cum - (rng[:, :, 1] - rng[:, :, 0]), 1, p)
        pos = torch.gather(rng[:, :, 0], 1, p) + (j - first)
        cand = self._perm[torch.where(ok, pos, torch.zeros_like(pos))].to(torch.int64)
        return torch.where(ok, cand, torch.full_like(cand, -1)), ok

    def _search_large_k_cells(self, q, k, valid, cells, max_probed):
        """k > 64: exact distances and a keyed top-k (``_keyed_topk``) over each query's probed rows, in query chunks.  Correct,
        not tuned: a wave per (query, probed row)."""
        N = self._n_rows
        vb = self._unpack_bits(valid, N)
        R = max(max_probed, 1)
        kk = min(k, R)
        chunk = max(1, min(q.shape[0], (1 << 25) // R))
        out = []
        for b0 in range(0, q.shape[0], chunk):
            cand, ok = self._probed_rows(cells[b0:b0 + chunk], R)
            ok = ok & vb[cand.clamp(min=0)]
            out.append(self._keyed_topk(q[b0:b0 + chunk].contiguous(), cand, ok, kk))
        d, i = pad_to_k(torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out]), k)
        if self.metric == Metric.EUCLIDEAN:
            d = torch.sqrt(d)
        return d, i
