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
  * sealed view, rebuilt lazily after a mutation (one sort over the live rows):
      ``_perm``       i32 [n_live]  the live offsets grouped by cell, ascending inside a cell
      ``_cell_rows``  i64 [C, 2]    (begin, end) of every cell in ``_perm``
      ``_cell_order`` i32 [C]       cells by descending size
      on the host: the cells' lengths in descending order, summed from the largest on (``_sizes_cum``): the largest cell and the
      sum of the P largest are the two numbers the search call wants
"""
from typing import Optional

import torch

from ... import ops
from ...enums import Metric
from ..codec.vq import VQCodec
from .cells import CellColumnMixin
from .flat_gpu import FlatGpuIndex, is_f16
from .row_store import empty_answer, like_input, pad_to_k


class IvfFlatGpuIndex(CellColumnMixin, FlatGpuIndex):
    FORMAT = 'annlite_amd.IvfFlatGpuIndex/1'

    def __init__(self, dim: int, vq_codec: Optional[VQCodec] = None, n_probe: Optional[int] = None, metric: Metric = Metric.COSINE,
                 **kwargs):
        assert vq_codec is not None, 'IvfFlatGpuIndex needs a VQCodec'
        self.vq_codec = vq_codec
        self.n_probe = n_probe  # None: every cell (the reference's behaviour)
        self._sealed = False
        self._perm = self._cell_rows = self._cell_order = self._sizes_cum = None
        # (accepted and ignored: the cell-tile filter is the f32 one, and so is this index's every-cell search -- the split filter
        # over cell tiles is not built)
        kwargs.pop('flat_filter', None)
        kwargs.pop('centre', None)
        if is_f16(kwargs.get('dtype', 'float32')):
            raise NotImplementedError('dtype=np.float16: the cell-tile kernels read f32 rows only (half-precision rows exist in the '
                                      'exhaustive FlatGpuIndex: no graph, n_cells=1)')
        super().__init__(dim, metric=metric, **kwargs)

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
    def search_batch(self, x, limit: int = 10, indices=None, n_probe: Optional[int] = None):
        """``FlatGpuIndex.search_batch`` over the rows of each query's ``n_probe`` nearest cells (every cell: that search itself)."""
        P = self.n_probe if n_probe is None else n_probe
        C = self.n_cells
        if P is None or P >= C:
            return super().search_batch(x, limit=limit, indices=indices)
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
            if k <= 64:
                d, i = ops.ivf_flat_search_topk(int(self.metric), q, self._vectors, self._norms, cells, C, self._perm, self._cell_rows,
                                                self._cell_order, max_cell, max_probed, k, valid_bits=valid, n_rows=self._n_rows,
                                                sqrt=self.metric == Metric.EUCLIDEAN, workspace=self._ws)  # hnsw/index.py:164-165
                self._overflowed = None  # (read from the workspace when asked for: it costs a synchronisation)
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
