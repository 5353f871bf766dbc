"""``GpuLevel0Graph`` -- the level-0 graph of the HNSW-over-PQ index BUILT ON THE GPU in batches (round 6; kernels:
``annlite_amd/csrc/graph_build.hip``; the searches of an insertion are the same packed pair walk queries use, ``graph.hip``).

What it replaces: hnswlib ``addPoint`` (include/hnswlib/hnswalg.h:1108-1235) as ``HnswIndex.add_with_ids`` drives it
(annlite/core/index/hnsw/index.py:124-137), in the form ``libannlite_graph.so`` restates it (hnsw_host.cpp ``insert`` /
``select_neighbors`` / ``connect``): search with ``ef_construction``, keep at most ``max_connection`` candidates by the
diversification heuristic (Algorithm 4) under the symmetric code-to-code L2 distance, link back with a shrink to
``2 * max_connection``.  Same knobs, same rules -- for a BATCH of points at a time:

  * a graph of fewer than ``BRUTE`` (8192) nodes grows by exact candidate lists: the ``ef_construction`` nearest stored points of
    every new point (ADC distance: the point's vector against the DECODED rows), batch mates included -- one ``cdist``;
  * beyond that a batch is ``min(16384, nodes / 4)`` points: their L2 tables (``annlite_lut_build``) are the queries of ONE packed
    pair walk over the graph as it is, ``annlite_graph_build_select`` writes their lists, the (target, source) pairs are sorted on
    the device and ``annlite_graph_build_reverse`` updates every target once, ``annlite_graph_pack_nodes`` re-packs the records
    that changed.  The points of a batch do not see each other (they meet through the neighbours both link to and through later
    batches' reverse links); a batch is at most a quarter of the graph while it is small and 16384 points later (0.3 % at 5M).

Only level 0 exists: the GPU walk scans a seed sample flat instead of descending upper layers (graph.hip), so none are built --
``seeds()`` is up to 128 nodes spread evenly over the insertion order.

Two distance backends share the batching, the seeds, the pair sort and the persistence (``Level0GraphBase``):

  * ``GpuLevel0Graph`` -- the PQ backend described above: code rows, the symmetric code-to-code table, packed node records;
  * ``GpuLevel0GraphF32`` -- the float backend (``graph_f32.hip``): every distance is
    ``annlite_exact_gather_dist``'s for the metric, between rows of the index's OWN vector column -- it holds no codes, no packed
    records and no second copy of the vectors; below ``BRUTE`` nodes the candidate lists come from one torch product in the metric's
    order (the select kernel recomputes every distance it compares: only the visiting order is torch's).
"""
from typing import Optional, Tuple

import torch

from ... import ops
from ..._capi import LAYOUT_BMK, LUT_L2
from ...enums import Metric


class Level0GraphBase:
    """What the two backends share: the link lists, batching (``BRUTE`` / ``BATCH`` / ``GROW``), ``seeds()``, the pair sort between the
    select and the reverse kernel, ``state()`` / ``load_state()``.  A backend provides ``_exact_candidates``, ``_walk_candidates``,
    ``_select``, ``_reverse`` and, where it keeps more than the lists, ``_grow_columns`` / ``_lists_changed``."""
    BRUTE = 8192       # below this many nodes: exact candidate lists
    BATCH = 16384      # points per walk batch
    GROW = 4           # ... and at most 1 / GROW of the graph (while it is small)
    MAX_SEEDS = 128    # seeds the walk scans flat (5M rows: 32 ... 1024 seeds give the same recall, 1024 cost 16 rounds of 64 per query)

    def __init__(self, device, max_connection: int = 16, ef_construction: int = 200):
        assert 2 <= max_connection <= 16, 'the GPU graph build holds 2 * max_connection <= 32 links per node'
        self.device = device
        self.Mc = int(max_connection)
        self.lpn = 2 * self.Mc
        self.efc = int(min(max(ef_construction, self.Mc), 256))
        self.n = 0
        self.links = None
        self._seeds: Optional[Tuple[int, torch.Tensor]] = None

    # ------------------------------------------------------------------ storage
    def reserve(self, cap: int):
        cur = 0 if self.links is None else self.links.shape[0]
        if cap <= cur:
            return
        cap = max(cap, cur * 2, 1024)
        links = torch.zeros((cap, self.lpn + 1), dtype=torch.int32, device=self.device)
        if self.n:
            links[: self.n] = self.links[: self.n]
        self._grow_columns(cap)
        self.links = links

    def _grow_columns(self, cap: int):
        """re-allocate the backend's own ``[cap, ...]`` columns, keeping their first ``self.n`` rows"""

    def seeds(self) -> torch.Tensor:
        """Up to ``MAX_SEEDS`` distinct nodes spread evenly over the insertion order (i32)."""
        if self._seeds is None or self._seeds[0] != self.n:
            n, s = self.n, min(self.n, self.MAX_SEEDS)
            idx = (torch.arange(s, device=self.device, dtype=torch.int64) * n) // max(s, 1)
            self._seeds = (n, idx.to(torch.int32).contiguous())
        return self._seeds[1]

    # ------------------------------------------------------------------ build
    def _insert(self, n_new: int):
        """Link the ``n_new`` points the backend has stored as nodes ``self.n .. self.n + n_new`` (``pos``: offset into them)."""
        pos = 0
        while pos < n_new:
            n = self.n
            if n < self.BRUTE:
                b = min(n_new - pos, self.BRUTE - n)
                cand = self._exact_candidates(pos, n, b)
            else:
                b = min(n_new - pos, self.BATCH, max(1024, n // self.GROW))
                cand = self._walk_candidates(pos, n, b)
            self._link(cand, n, b)
            pos += b

    def _link(self, cand: torch.Tensor, n: int, b: int):
        pairs = self._select(cand.contiguous(), n, b)
        keys = torch.sort(pairs.reshape(-1)).values
        n_keys = int((keys != torch.iinfo(torch.int64).max).sum().item())
        new_nodes = torch.arange(n, n + b, device=keys.device, dtype=torch.int64)
        if n_keys:
            keys = keys[:n_keys].contiguous()
            targets, counts = torch.unique_consecutive(keys >> 32, return_counts=True)
            seg = torch.zeros((targets.numel() + 1,), dtype=torch.int64, device=keys.device)
            seg[1:] = torch.cumsum(counts, 0)
            self._reverse(keys, seg, n + b)
            changed = torch.cat([targets, new_nodes])
        else:
            changed = new_nodes
        self.n = n + b
        self._lists_changed(changed)

    def _lists_changed(self, nodes: torch.Tensor):
        """the lists of ``nodes`` i64 were rewritten (``self.n`` counts the batch already)"""

    # ------------------------------------------------------------------ persistence
    def state(self):
        return {'n': self.n, 'links': self.links[: self.n].cpu().numpy() if self.n else None}

    def _load_links(self, st) -> int:
        n = int(st['n'])
        self.n = 0
        self.links = None
        self._seeds = None
        if n:
            self.reserve(n)
            self.links[:n] = ops.to_dev(st['links'], dev=self.device)
            self.n = n
        return n


class GpuLevel0Graph(Level0GraphBase):
    """The PQ backend: PQLookup walks over packed records, Algorithm 4 under the symmetric code-to-code table."""

    def __init__(self, codebooks_dev: torch.Tensor, max_connection: int = 16, ef_construction: int = 200):
        M, Ks, dsub = codebooks_dev.shape
        assert M in (8, 16, 32, 64) and Ks <= 256, 'the GPU graph build supports M in {8, 16, 32, 64} and uint8 codes'
        super().__init__(codebooks_dev.device, max_connection, ef_construction)
        self.cb = codebooks_dev.contiguous()
        self.M, self.Ks, self.dsub = M, Ks, dsub
        self.sdc = ops.graph_build_sdc(self.cb)
        self.rec = ops.graph_record_bytes(self.lpn, M)
        self.codes = self.packed = None
        self._x = None

    def _grow_columns(self, cap: int):
        codes = torch.zeros((cap, self.M), dtype=torch.uint8, device=self.device)
        packed = torch.zeros((cap, self.rec), dtype=torch.uint8, device=self.device)
        if self.n:
            codes[: self.n] = self.codes[: self.n]
            packed[: self.n] = self.packed[: self.n]
        self.codes, self.packed = codes, packed

    def add(self, x: torch.Tensor, codes: torch.Tensor):
        """Insert ``x`` f32 [n, D] (what the walk's tables are built from: pre-processed vectors) with their PLAIN code rows u8 [n, M];
        the points become nodes ``self.n .. self.n + n``."""
        n_new = x.shape[0]
        if n_new == 0:
            return
        assert codes.shape == (n_new, self.M) and codes.dtype == torch.uint8
        self.reserve(self.n + n_new)
        self.codes[self.n: self.n + n_new] = codes
        self._x = x
        try:
            self._insert(n_new)
        finally:
            self._x = None

    def _exact_candidates(self, pos: int, n: int, b: int) -> torch.Tensor:
        """The ``ef_construction`` nearest of the n + b stored points (batch mates included, the point itself not) for each of the b
        new points, ascending: ADC distance as |x - decode(row)|^2."""
        x = self._x[pos: pos + b]
        total = n + b
        xhat = ops.pq_decode(self.codes[:total], self.cb)
        d = torch.cdist(x.to(torch.float32), xhat).square_()
        d[torch.arange(b, device=d.device), torch.arange(n, total, device=d.device)] = float('inf')
        k = min(self.efc, total - 1)
        cand = torch.full((b, self.efc), -1, dtype=torch.int64, device=d.device)
        if k > 0:
            cand[:, :k] = torch.topk(d, k, dim=1, largest=False, sorted=True).indices
        return cand

    def _walk_candidates(self, pos: int, n: int, b: int) -> torch.Tensor:
        lut = ops.lut_build(self._x[pos: pos + b].contiguous(), self.cb, LUT_L2, LAYOUT_BMK)
        cand, _ = ops.graph_search_packed(self.packed, self.lpn, self.seeds(), self.codes, lut, self.efc, n_rows=n, expand_width=2)
        return cand

    def _select(self, cand: torch.Tensor, n: int, b: int) -> torch.Tensor:
        return ops.graph_build_select(cand, n, self.codes, self.sdc, self.Mc, self.links)

    def _reverse(self, keys: torch.Tensor, seg: torch.Tensor, n_after: int):
        ops.graph_build_reverse(keys, seg, self.codes, self.sdc, self.links)

    def _lists_changed(self, nodes: torch.Tensor):
        ops.graph_pack_nodes(self.links, self.codes, nodes.contiguous(), self.packed, self.n)

    def load_state(self, st, codes: torch.Tensor):
        """``codes``: the PLAIN code rows of nodes 0..n (the index's own table)."""
        self.codes = self.packed = None
        n = self._load_links(st)
        if n == 0:
            return
        self.codes[:n] = codes[:n]
        ops.graph_pack_nodes(self.links, self.codes, torch.arange(n, device=self.device, dtype=torch.int64), self.packed, n)


class GpuLevel0GraphF32(Level0GraphBase):
    """The float backend: ``annlite_graph_f32_search`` / ``_build_select`` / ``_build_reverse`` over the rows of a vector column the
    CALLER owns (``add(vectors, n_new)``: rows ``self.n .. self.n + n_new`` of ``vectors`` are stored already).  ``metric``: the C
    ABI's number; COSINE rows arrive normalised."""

    def __init__(self, device, metric: int, max_connection: int = 16, ef_construction: int = 200):
        super().__init__(device, max_connection, ef_construction)
        self.metric = int(metric)
        self._v = None

    def add(self, vectors: torch.Tensor, n_new: int):
        if n_new == 0:
            return
        assert vectors.dtype == torch.float32 and vectors.is_contiguous() and vectors.shape[0] >= self.n + n_new
        self.reserve(self.n + n_new)
        self._v = vectors
        try:
            self._insert(int(n_new))
        finally:
            self._v = None

    def _exact_candidates(self, pos: int, n: int, b: int) -> torch.Tensor:
        """The ``ef_construction`` nearest of the n + b stored rows (batch mates included, the point itself not), ascending in the
        metric's order: squared L2 (COSINE rows are normalised: the same order), or minus the inner product."""
        total = n + b
        rows, x = self._v[:total], self._v[n: total]
        if self.metric == int(Metric.INNER_PRODUCT):  # 1 - <q, x> ascends as <q, x> descends
            d = -(x @ rows.T)
        else:
            d = torch.cdist(x, rows).square_()
        d[torch.arange(b, device=d.device), torch.arange(n, total, device=d.device)] = float('inf')
        k = min(self.efc, total - 1)
        cand = torch.full((b, self.efc), -1, dtype=torch.int64, device=d.device)
        if k > 0:
            cand[:, :k] = torch.topk(d, k, dim=1, largest=False, sorted=True).indices
        return cand

    def _walk_candidates(self, pos: int, n: int, b: int) -> torch.Tensor:
        cand, _ = ops.graph_f32_search(self.metric, self._v[n: n + b], self._v, self.links, self.seeds(), self.efc, n_rows=n)
        return cand

    def _select(self, cand: torch.Tensor, n: int, b: int) -> torch.Tensor:
        return ops.graph_f32_build_select(self.metric, cand, n, self._v, self.Mc, self.links, n_rows=n + b)

    def _reverse(self, keys: torch.Tensor, seg: torch.Tensor, n_after: int):
        ops.graph_f32_build_reverse(self.metric, keys, seg, self._v, self.links, n_rows=n_after)

    def load_state(self, st):
        self._load_links(st)
