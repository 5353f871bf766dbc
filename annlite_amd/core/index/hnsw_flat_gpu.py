"""``HnswFlatGpuIndex`` -- a level-0 HNSW graph over the un-quantised float vectors, built and walked on the GPU: the sub-linear form of
the reference's default configuration (``AnnLite(n_dim)`` without ``n_subvectors`` is ``HnswIndex`` on float vectors,
annlite/core/index/hnsw/index.py:52-191; same knobs: ``max_connection`` 16, ``ef_construction`` 200, ``ef_search`` 50).

It IS a ``FlatGpuIndex`` -- same rows, norms, validity bitmap, exact ``search_exhaustive`` -- with link lists beside the rows:

  * built in batches by ``graph_gpu_build.GpuLevel0GraphF32`` (``graph_f32.hip``), which reads this index's own
    ``_vectors`` column: no second copy of the vectors;
  * walked by ``annlite_graph_f32_search``, one wave per query.  Every distance of build and walk carries
    ``annlite_exact_gather_dist``'s bits for the metric -- the numbers ``FlatGpuIndex`` returns -- so the walk's list is final: no
    re-rank, a stored vector found by its own query comes back at exactly 0.0, and an id both indexes return carries the same bits.
    As in hnswlib's spaces the graph is built and walked with the metric's own distance (COSINE rows are stored normalised: the L2
    order; INNER_PRODUCT walks ``1 - <q, x>``).

A search the graph does not serve -- k or ef beyond 256, no graph yet, and by default a filter (``indices=``) -- is answered by the
exact search of the parent: never worse.  ``filter_search='graph'`` (constructor, or per call) answers a filtered search on the graph
instead, as hnswlib's ``searchBaseLayerSTWithFilter`` does: ``annlite_graph_f32_search_admit`` walks through every node and keeps the
best admitted rows among everything it evaluates ("filtered walk").  Ids must be dense in insertion order
(0, 1, 2, ...: what AnnLite's offsets are); rows are not updated in place (delete + add a new offset, hnsw/index.py:173-177); a delete
clears the validity bit only -- the row keeps routing the walk.  ``flat_filter`` / ``centre`` / ``filter_route`` are the parent's keywords
and reach it unchanged: they choose the filter of those exact searches (``search_exhaustive`` included) and whether a filtered one scans
the table or the selected rows, never the walk.
"""
from pathlib import Path
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from ... import ops
from ...enums import Metric
from .filter_walk import FilterWalkMixin
from .flat_gpu import FlatGpuIndex, is_f16, is_i8
from .row_store import RowStoreIndex, empty_answer, like_input, ranked_answer


class HnswFlatGpuIndex(FilterWalkMixin, FlatGpuIndex):
    FORMAT = 'annlite_amd.HnswFlatGpuIndex/1'
    ALSO_LOADS = (FlatGpuIndex.FORMAT,)  # (rows without links: the graph is rebuilt from them)
    MAX_EF = 256                         # the walk's list: four registers per lane
    MAX_DIM = 2048
    # (a filter per query: one search_batch per group -- the graph search stays the search it is under every selection)
    search_batch_grouped = RowStoreIndex.search_batch_grouped
    # DESIGN.md section 3.8, table "filtered walk" (1M x 128): the smallest measured share of admitted rows at which the filtered walk
    # is faster than the exact filtered search AND within 0.03 of the unfiltered walk's recall@10 (at 0.05 a sixth of the queries is
    # answered again exactly and the two paths are level: 211 k against 220 k q/s)
    FILTER_WALK_MIN_FRACTION = 0.1

    def __init__(self, dim: int, dtype: np.dtype = np.float32, metric: Metric = Metric.COSINE, ef_construction: int = 200,
                 ef_search: int = 50, max_connection: int = 16, seed: int = 100, build: Optional[str] = 'gpu',
                 index_file: Optional[Union[str, Path]] = None, filter_search: str = 'exact', **kwargs):
        # (named here: RowStoreIndex drops the HNSW kwargs the reference forwards to every index)
        if build not in (None, 'gpu'):
            raise NotImplementedError(f"build={build!r}: only the GPU-built level-0 graph exists over float vectors (build='gpu')")
        if not 2 <= int(max_connection) <= 16:
            raise ValueError(f'max_connection={max_connection}: the GPU graph holds 2 * max_connection <= 32 links per node (2 ... 16)')
        if not 1 <= int(dim) <= self.MAX_DIM:
            raise ValueError(f'dim={dim}: the float graph takes 1 <= dim <= {self.MAX_DIM}')
        self._check_filter_search(filter_search, "the parent's exact filtered search")
        if is_f16(dtype):
            raise NotImplementedError('dtype=np.float16: the float graph walks and builds over f32 rows only (half-precision rows exist '
                                      'in the exhaustive FlatGpuIndex: no graph, n_cells=1)')
        if is_i8(dtype):
            raise NotImplementedError('dtype=np.int8: the float graph walks and builds over f32 rows only (int8 rows exist '
                                      'in the exhaustive FlatGpuIndex: no graph, n_cells=1)')
        super().__init__(dim, dtype=dtype, metric=metric, **kwargs)
        self.ef_construction = int(ef_construction)  # hnsw/index.py:66-69
        self.ef_search = int(ef_search)
        self.max_connection = int(max_connection)
        self.seed = int(seed)  # (kept for the reference's signature: level 0 only -- no random level is drawn)
        self.build = 'gpu'
        self._init_filter_search(filter_search)
        self._gg = None  # GpuLevel0GraphF32
        if index_file:
            self.load(index_file)

    # ------------------------------------------------------------------ graph handle
    def _ensure_graph(self):
        if self._gg is None:
            from .graph_gpu_build import GpuLevel0GraphF32

            self._gg = GpuLevel0GraphF32(self._device(), int(self.metric), self.max_connection, self.ef_construction)
        return self._gg

    def _rebuild_graph(self, N: int):
        """Link rows 0 .. N of the vector column from nothing."""
        self._gg = None
        if N:
            gg = self._ensure_graph()
            gg.reserve(int(self.capacity))
            gg.add(self._vectors, N)

    # ------------------------------------------------------------------ build
    def add_with_ids(self, x, ids: List[int], **kwargs):
        ids_np = np.ascontiguousarray(np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids, dtype=np.int64)).reshape(-1)
        if ids_np.size == 0:
            return
        n = self._n_rows
        if not (ids_np[0] == n and (np.diff(ids_np) == 1).all()):
            raise RuntimeError(f'the GPU-built graph takes ids in insertion order (next: {n}, got {ids_np[:3]}...)')
        super().add_with_ids(x, ids_np)  # rows, norms, validity (the parent pre-processes; it may re-allocate the columns)
        gg = self._ensure_graph()
        if gg.n != n:  # (rows without links -- a graph dropped behind the rows' back: link them all)
            self._rebuild_graph(self._n_rows)
            return
        gg.reserve(int(self.capacity))
        gg.add(self._vectors, ids_np.size)

    def update_with_ids(self, x, ids: List[int], **kwargs):
        raise RuntimeError('the HNSW graph does not support in-place updates (delete + add a new offset): '
                           'hnsw/index.py:173-177')

    def reset(self, capacity: Optional[int] = None):
        super().reset(capacity=capacity)
        self._gg = None

    # ------------------------------------------------------------------ search
    def candidates(self, q_dev: torch.Tensor, ef: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Graph walk for pre-processed queries ``q_dev`` f32 [B, D]: ``(ids i64 [B, ef], distance f32 [B, ef])`` on the device,
        ascending by (distance, id); deleted rows blanked in place to (-1, +inf).  The distances are the metric's own, final (squared
        for EUCLIDEAN)."""
        ef = int(ef or self.ef_search)
        gg = self._gg
        if gg is None or gg.n == 0 or gg.n != self._n_rows:
            raise RuntimeError('no graph to walk (the index is empty)')
        if ef > self.MAX_EF:
            raise RuntimeError(f'the GPU walk keeps ef <= {self.MAX_EF} candidates (ef = {ef})')
        return ops.graph_f32_search(int(self.metric), q_dev.contiguous(), self._vectors, gg.links, gg.seeds(), ef,
                                    valid_bits=self._valid, n_rows=gg.n)

    def search_exhaustive(self, x, limit: int = 10, **kw):
        return super().search_batch(x, limit=limit, **kw)

    # the filtered walk's two hooks (filter_walk.FilterWalkMixin)
    def _filter_walk(self, q, ef_route: int, ef: int, admit, reach):
        gg = self._gg
        return ops.graph_f32_search_admit(int(self.metric), q.contiguous(), self._vectors, gg.links, gg.seeds(), ef_route, ef, admit,
                                          n_rows=gg.n, route_worst=reach)

    def _filter_rank(self, x, q, cand, cand_d, k: int, ef: int, admit):
        # (the list is ascending with its missing places at the tail: the first k columns are the answer, by position)
        pos = torch.arange(k, device=q.device, dtype=torch.int64)[None, :].expand(q.shape[0], k)
        return (*ranked_answer(cand, cand_d[:, :k], pos, k, sqrt=self.metric == Metric.EUCLIDEAN), k)

    def search_batch(self, x, limit: int = 10, indices=None, ef_search: Optional[int] = None, filter_search: Optional[str] = None,
                     **kwargs):
        """``(dists [B, k], ids [B, k])``: the first k real entries of the walk's list of ``max(ef_search, k)`` candidates.  An index
        without a graph and k or ef beyond 256 are answered by the parent's exact search, and so is a filter (``indices``) unless
        ``filter_search`` -- this call's, else the constructor's -- is ``'graph'``.

        ``filter_search='graph'``: the walk of ``annlite_graph_f32_search_admit`` routes through every node and lists admitted rows
        only.  Set on the constructor it is a rule -- filters that admit less than ``FILTER_WALK_MIN_FRACTION`` of the rows still go
        to the exact search, where the walk does not pay --; given per call it is an order.  A query whose list ends with fewer than
        ``min(k, admitted rows)`` entries is answered again by the exact filtered search, so a filtered search through the graph
        never returns fewer rows than the exact one; and so is a query whose k-th row lies beyond the distance of the routing
        list's last place -- the walk did not reach that far, it only met such rows on the way (a filter that admits nothing near
        the query).  Finding those queries costs one host look at a column of the walk's result.
        ``last_filter_path`` ('graph' / 'exact') and ``last_filter_reanswered`` say what the last filtered search did."""
        self._check_filter_search(filter_search)
        k = int(limit)
        ef = max(int(ef_search or self.ef_search), k)
        gg = self._gg
        no_walk = gg is None or gg.n == 0 or gg.n != self._n_rows or k > self.MAX_EF or ef > self.MAX_EF
        if indices is not None:
            self._overflowed, self.last_flat_filter, self.last_filter_route = 0, None, None  # (a walk runs no filter; the parent's search sets its own)
            answer = self._filtered_answer(x, k, ef, indices, filter_search, not no_walk)
            if answer is not None:
                return answer
        if indices is not None or no_walk:
            return super().search_batch(x, limit=limit, indices=indices, filter_route=kwargs.get('filter_route'))
        is_np = not isinstance(x, torch.Tensor)
        q = self._pre(x)
        B = q.shape[0]
        self._overflowed = 0
        self.last_flat_filter = self.last_filter_route = None  # (a walk: no filter ran, no table was scanned)
        if B == 0:
            return like_input(is_np, *empty_answer(B, k, q.device))
        cand, cand_d = self.candidates(q, ef)
        if k <= 64:
            d, pos = ops.topk_rows(cand_d, min(k, ef))
        else:  # (beyond the wave kernel's k: a stable sort keeps the (value, position) order)
            sd, si = torch.sort(cand_d, dim=1, stable=True)
            d, pos = sd[:, :k], torch.where(torch.isinf(sd[:, :k]), torch.full_like(si[:, :k], -1), si[:, :k])
        return like_input(is_np, *ranked_answer(cand, d, pos, k, sqrt=self.metric == Metric.EUCLIDEAN))

    # ------------------------------------------------------------------ persistence: the links ride in the row store's one envelope
    def _dump_state(self, N):
        st = super()._dump_state(N)
        gg = self._gg
        if gg is not None and gg.n == N and N:
            st['links'] = gg.links[:N].cpu().numpy()
            st['max_connection'] = self.max_connection
        return st

    def _load_state(self, state, N):
        super()._load_state(state, N)
        self._gg = None
        links = state.get('links')
        if N and links is not None and links.shape == (N, 2 * self.max_connection + 1):
            self._ensure_graph().load_state({'n': N, 'links': links})
        elif N:
            # rows without (usable) links -- the flat index's file, or lists of another max_connection: rebuilt from the stored rows
            self._rebuild_graph(N)
