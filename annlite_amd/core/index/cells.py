"""``CellColumnMixin`` -- what the indexes over coarse cells share (``IvfPQGpuIndex``, ``IvfFlatGpuIndex``): the ``_cell_of``
column of the row store, its assignment at add / update from the vectors as given, which cells a query probes, and the
``.cells.npy`` side file of ``dump`` / ``load``.  How the cells are laid out for a search (the sealed view) is each index's own:
every mutation here only clears ``_sealed``.

Mixed in FRONT of a ``RowStoreIndex``; the index sets ``vq_codec`` and ``_sealed`` before the row store's constructor runs.
"""
from typing import Optional, Tuple

import numpy as np
import torch

from ... import ops
from ...enums import Metric


class CellColumnMixin:
    @property
    def n_cells(self) -> int:
        return self.vq_codec.n_clusters

    # ------------------------------------------------------------------ storage
    def _columns(self):
        return {**super()._columns(), '_cell_of': ((), torch.int32)}  # (a column: a growth carries the cells along)

    def _alloc(self, capacity: int):
        super()._alloc(capacity)
        self._sealed = False  # (new storage, whoever asked for it: the sealed view is of the old one)

    def add_with_ids(self, x, ids, **kwargs):
        ids_t = self._ids_to_dev(ids)
        if ids_t.numel() == 0:
            return
        super().add_with_ids(x, ids_t)  # rows / validity exactly as the index without cells stores them
        # the reference assigns cells on the vectors as given (index.py:291-292, vq.py:81-90)
        raw = ops.to_dev(x, torch.float32)
        raw = raw.reshape(1, -1) if raw.ndim == 1 else raw
        self._cell_of[ids_t] = self.vq_codec.encode(raw).to(torch.int32)
        self._sealed = False

    def delete(self, ids):
        super().delete(ids)
        self._sealed = False

    def reset(self, capacity: Optional[int] = None):
        super().reset(capacity=capacity)
        self._sealed = False

    # ------------------------------------------------------------------ cell selection
    def _select_kind_and_centroids(self) -> Tuple[int, torch.Tensor]:
        """cdist(query, vq codebook, metric) of ``_cell_selection`` (index.py:462-464) as a ranking."""
        cb = self.vq_codec.codebook_dev
        if self.metric == Metric.EUCLIDEAN:
            return 0, cb
        if self.metric == Metric.COSINE:
            return 1, ops.l2_normalize(cb)  # queries are normalised by _pre: 1 - cos ranks like -<q, c/|c|>
        return 1, cb

    def probe_cells(self, q: torch.Tensor, n_probe: int) -> torch.Tensor:
        kind, cent = self._select_kind_and_centroids()
        return ops.ivf_select_cells(kind, q, cent, n_probe)

    # ------------------------------------------------------------------ persistence
    def dump(self, index_file):
        super().dump(index_file)
        np.save(str(index_file) + '.cells.npy', self._cell_of[: self._n_rows].cpu().numpy())

    def load(self, index_file):
        super().load(index_file)
        cells = np.load(str(index_file) + '.cells.npy')
        self._cell_of[: cells.shape[0]] = ops.to_dev(cells)
        self._sealed = False
