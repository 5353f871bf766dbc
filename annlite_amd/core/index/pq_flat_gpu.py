"""``PQFlatGpuIndex`` -- exhaustive PQ/ADC index on one MI355X, plugging in where the reference
constructs ``HnswIndex(pq_codec=...)`` per cell (annlite/container.py:48-59).

Semantics = the reference's flat ADC index ``PQIndex`` (annlite/core/index/pq_index.py:11-56) made
metric-aware and batched, with ``HnswIndex``'s pre/post-processing so it is a drop-in for the seam
``CellContainer`` uses (SURVEY.md section 8b "Index plugin seam"):

  * ``search(x[D], limit, indices)`` -> ``(dists[k], ids[k])`` ascending        hnsw/index.py:139-167
      reshape to (1, D), cast f32, ``l2_normalize`` if cosine (index.py:28-29), tables through
      ``PQCodec.get_dist_mat`` (which normalises again, pq.py:309-310), ``sqrt`` of the distances
      for EUCLIDEAN (index.py:164-165); cosine / inner product distances are ``M/Ks - <q, x^>``.
  * ``add_with_ids(data[N,D], offsets)``   encode + store rows at ``offsets``      hnsw/index.py:124-137
  * ``delete(ids)``  marks rows (never returned again)                            hnsw/index.py:169-171
  * ``reset`` / ``dump`` / ``load`` / ``size`` / ``capacity``                      hnsw/index.py:116-122,185-191
  * untrained codec -> ``RuntimeError('Please train the PQ ...')``                hnsw/index.py:32-35
plus ``search_batch(X[B,D], limit)`` so that a whole ``AnnLite.search(docs)`` call is one launch
instead of the reference's per-query python loop (annlite/container.py:214).

Storage, validity, the mutation protocol, ``search`` and the file envelope are ``RowStoreIndex``'s (row_store.py), shared with
``FlatGpuIndex``; this module declares the columns, writes them (SKEWED where the fast scan plan applies) and searches them.

Data layout in HBM: one ``uint8 [capacity, M]`` code table, stored pre-SKEWED (row n
rotated left by n mod M bytes) when the fast scan plan applies; a ``uint32`` validity bitmap (delete
marks / never-written rows); optionally the raw ``float32 [capacity, D]`` vectors for the exact
re-rank stage (``rerank=True``; 10M x 128 fp32 = 5.1 GB of the 288 GB).
"""
from pathlib import Path
from typing import Optional, Tuple, Union

import numpy as np
import torch

from ... import ops
from ..._capi import CODES_PLAIN, CODES_SKEWED, ScanState, scan_plan
from ...enums import ExpandMode, Metric
from ...math import l2_normalize_host
from ..codec.pq import PQCodec
from .row_store import RowStoreIndex, empty_answer, float_from_key, float_order_key, like_input, pad_to_k, ranked_answer


class SplitBatch:
    """A batch between the two halves of the split search (``PQFlatGpuIndex.split_prepare``; protocol: sharded.py)."""

    def __init__(self, keys, n_queries, device, union, scan, plain, keep=None):
        self.keys, self.n_queries, self.device = keys, n_queries, device
        self.union, self.scan, self.plain, self._keep = union, scan, plain, keep


class PQFlatGpuIndex(RowStoreIndex):
    FORMAT = 'annlite_amd.PQFlatGpuIndex/1'
    STATE_KEYS = ('dim', 'M', 'Ks')

    def __init__(
        self,
        dim: int,
        pq_codec: Optional[PQCodec] = None,
        dtype: np.dtype = np.float32,
        metric: Metric = Metric.COSINE,
        rerank: bool = False,
        skewed: bool = True,
        index_file: Optional[Union[str, Path]] = None,
        rerank_pool: str = 'slices',
        **kwargs,
    ):
        assert pq_codec is not None, 'PQFlatGpuIndex needs a PQCodec'
        self.pq_codec = pq_codec  # (before the base class asks for the columns: they follow the codec)
        self.rerank = bool(rerank)
        super().__init__(dim, dtype=dtype, metric=metric, **kwargs)
        # candidates of the exact re-rank stage: 'slices' = the union of the row slices' own ADC top-rerank_k lists (n_slices x
        # rerank_k rows); 'global' = the global ADC top-rerank_k (<= 64, default 50) of the shared-bound search
        assert rerank_pool in ('slices', 'global')
        self.rerank_pool = rerank_pool
        self._want_skew = bool(skewed)
        self._ws = ops.ScanWorkspace()
        self._scan_state = None  # the library's per-table kernel choice (created with the device storage)
        if index_file:
            self.load(index_file)

    # ------------------------------------------------------------------ storage
    @property
    def M(self) -> int:
        return self.pq_codec.n_subvectors

    @property
    def Ks(self) -> int:
        return self.pq_codec.n_clusters

    @property
    def code_bytes(self) -> int:
        return np.dtype(self.pq_codec.code_dtype).itemsize

    def _layout(self) -> int:
        fast = self.code_bytes == 1 and self.M in (8, 16, 32, 64) and self.Ks <= 256
        return CODES_SKEWED if (fast and self._want_skew) else CODES_PLAIN

    def _columns(self):
        """``uint8 [capacity, M]`` codes (wider for Ks > 256); the raw vectors only for the exact re-rank stage"""
        tdt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[self.code_bytes]
        return {'_codes': ((self.M,), tdt), '_vectors': ((self.dim,), torch.float32) if self.rerank else None}

    def _check_ready(self):
        if not self.pq_codec.is_trained:
            raise RuntimeError('Please train the PQ before using HNSW quantization backend')

    def _scan_inputs(self, x, q: torch.Tensor):
        """(LUT kind, queries as the table build sees them): ``PQCodec.get_dist_mat`` normalises cosine queries a second
        time (pq.py:309-310); for host buffers that happens on the host too, in the reference's arithmetic."""
        # (what the table build normalises is the CODEC's business -- pq.py:67-69 normalize_input --, not the index metric's)
        if isinstance(x, np.ndarray) and self.pq_codec.normalize_input:
            kind, _ = self.pq_codec.scan_inputs(q[:0])
            return kind, ops.to_dev(l2_normalize_host(l2_normalize_host(
                np.ascontiguousarray(x.reshape(1, -1) if x.ndim == 1 else x, dtype=np.float32))), torch.float32)
        return self.pq_codec.scan_inputs(q)

    # ------------------------------------------------------------------ mutation (protocol: row_store.py)
    def _write_rows(self, x, ids):
        codes = ops.pq_encode(x, self.pq_codec.codebooks_dev)
        if self._layout() == CODES_SKEWED:
            ops.codes_skew(codes, ids, out=self._codes)
        else:
            self._codes[ids] = codes
        if self._vectors is not None:
            self._vectors[ids] = x

    def reset(self, capacity: Optional[int] = None):
        super().reset(capacity=capacity)
        if self._scan_state is not None:
            self._scan_state.reset()

    # ------------------------------------------------------------------ kernel choice
    # Which M = 16 scan kernel serves this table -- byte filter tables (data with structure: what PQ is for) or u16 filter
    # tables (independent uniform codes: the byte filter leaks) -- is decided INSIDE the library, from what its own launches
    # measure (annlite_hip.h: annlite_scan_state): the first call(s) run the byte-table kernel guarded, later calls read
    # the verdict from the state's host-mapped block.  No calibration runs, no extra latency on a user's query, and
    # ANNLITE_SCAN_VARIANT in the environment still overrides everything for A/B measurements.
    @property
    def scan_state(self) -> ScanState:
        if self._scan_state is None:
            self._scan_state = ScanState()
        return self._scan_state

    @property
    def scan_kernel(self) -> str:
        """'undecided' | 'byte tables' | 'u16 tables' -- what the library has settled on for this table"""
        return ScanState.KERNELS[self.scan_state.info()[0]] if self._scan_state is not None else 'undecided'

    def search_batch(self, x, limit: int = 10, indices=None, rerank_k: Optional[int] = None, row_base: int = 0
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
        """All queries of ``x`` [B, D] in one launch.  Returns device tensors
        ``(dists f32 [B, k], ids i64 [B, k])``, ascending by (distance, id); missing -> (+inf, -1).
        With ``rerank=True`` indexes, the ADC scan produces ``n_slices * rerank_k`` candidates per query
        that are re-scored exactly on the stored float vectors."""
        is_np = not isinstance(x, torch.Tensor)
        q = self._pre(x)
        B = q.shape[0]
        k = int(limit)
        assert k >= 1
        N = self._n_rows
        valid = None
        if N > 0:
            valid = self._valid if indices is None else self._filter_bits(indices)
        dev = q.device
        if N == 0 or B == 0:
            d, i = empty_answer(B, k, dev)
        elif self.rerank and self._vectors is not None:
            d, i = self._search_rerank(q, k, valid, N, rerank_k, self._scan_inputs(x, q), filtered=indices is not None)
        elif k <= 64:
            # table build + scan + top-k: one C call (annlite_pq_search_topk)
            kind, xq = self._scan_inputs(x, q)
            base = row_base
            d, i = ops.pq_search_topk(
                kind, xq, self.pq_codec.codebooks_dev, self._codes, k, self.M, self.Ks, valid_bits=valid, n_rows=N,
                codes_layout=self._layout(), workspace=self._ws, row_base=base,
                sqrt=self.metric == Metric.EUCLIDEAN,  # hnsw/index.py:164-165
                state=self.scan_state if indices is None else None)  # (a filtered call says nothing about the table)
            row_base = 0
        else:
            d, i = self._search_large_k(q, k, valid, N, self._scan_inputs(x, q))
        if row_base:
            i = torch.where(i >= 0, i + row_base, i)  # (paths that do not take row_base natively)
        return like_input(is_np, d, i)

    def search_batch_packed(self, x, limit: int, row_base: int = 0) -> Optional[torch.Tensor]:
        """Plain ADC top-k of a device batch as ONE i64 tensor [B, k, 2] = (row_base + id or -1, bits of the RAW
        ADC sum -- no sqrt): the per-rank contribution to the single all-gather of the row-sharded search.
        ``None`` when this index state needs the general path (re-rank, k > 64)."""
        k = int(limit)
        if (self.rerank and self._vectors is not None) or k > 64:
            return None
        q = self._pre(x)
        B, N = q.shape[0], self._n_rows
        if N == 0 or B == 0:
            out = torch.empty((B, k, 2), dtype=torch.int64, device=q.device)
            out[..., 0] = -1
            out[..., 1] = 0x7F800000  # +inf
            return out
        kind, xq = self._scan_inputs(x, q)
        return ops.pq_search_topk(
            kind, xq, self.pq_codec.codebooks_dev, self._codes, k, self.M, self.Ks, valid_bits=self._valid,
            row_base=row_base, n_rows=N, codes_layout=self._layout(), workspace=self._ws, packed=True, state=self.scan_state)

    def split_supported(self, x, limit: int) -> bool:
        """STATIC part of the split search's conditions -- the same on every rank of a row-sharded search (configuration, batch
        shape, input kind), so that all ranks agree on whether the seed collective takes place at all."""
        k = int(limit)
        dsub = self.dim // self.M if self.M else 0
        return (isinstance(x, torch.Tensor) and x.ndim == 2 and x.shape[0] > 0 and not (self.rerank and self._vectors is not None) and
                1 <= k <= 16 and self.M == 16 and self.code_bytes == 1 and self.Ks <= 256 and self.dim <= 256 and dsub % 4 == 0 and
                self.metric == Metric.EUCLIDEAN and not self.pq_codec.normalize_input)

    def split_prepare(self, x, limit: int, row_base: int, seed_rows: int, workspace) -> Optional['SplitBatch']:
        """First half of ``search_batch_packed`` for a rank of a row-sharded search WITH a seed exchange (sharded.py runs the
        protocol): the preparation launch, seeding from this rank's first ``seed_rows`` rows only, into ``workspace`` (None: the index's own,
        per-stream scratch).  Returns the batch's handle -- ``keys`` i64 [B, 16] (this
        rank's contribution to the seed all-gather) or ``keys is None`` when the split does not apply to THIS rank NOW (fewer
        than 4096 rows, the library has not settled on the byte-table kernel yet: nothing was launched, ``plain()`` is the
        search) -- or ``None`` when ``split_supported`` says no (the same answer on every rank: no collective at all)."""
        from ..._capi import PHASE_PREPARE, PHASE_SCAN

        if not self.split_supported(x, limit):
            return None
        k = int(limit)
        q = self._pre(x)
        B = q.shape[0]
        kind, xq = self._scan_inputs(x, q)
        args = dict(valid_bits=self._valid, row_base=row_base, n_rows=self._n_rows, codes_layout=self._layout())
        workspace = workspace if workspace is not None else self._ws
        call = lambda phase, **kw: ops.pq_search_split(phase, kind, xq, self.pq_codec.codebooks_dev, self._codes, k, self.M, self.Ks,
                                                       self.scan_state, workspace, **args, **kw)
        keys = call(PHASE_PREPARE, seed_rows=seed_rows) if self._n_rows >= 4096 else None

        def union(all_keys):
            ops.pq_search_seed_union(all_keys.contiguous(), self._codes, B, k, self.M, self.Ks, workspace, n_rows=self._n_rows)

        return SplitBatch(keys=keys, n_queries=B, device=q.device, union=union, scan=lambda: call(PHASE_SCAN),
                          plain=lambda: self.search_batch_packed(x, limit, row_base), keep=(q, xq))

    @property
    def sqrt_epilogue(self) -> bool:
        """Metric epilogue of ``search`` on raw ADC sums (hnsw/index.py:164-165)."""
        return self.metric == Metric.EUCLIDEAN

    def _plain_codes(self, N: int) -> torch.Tensor:
        if self._layout() == CODES_SKEWED:
            return ops.codes_skew(self._codes[:N], inverse=True)
        return self._codes[:N]

    def _search_large_k(self, q, k, valid, N, scan_in=None):
        """k > 64 (beyond the scan kernels' lists): the distances of a CHUNK of queries to every row (adc_dist launches into one
        [chunk, N] buffer) -> i64 keys (order-preserving bits of the f32 sum << 32 | row: unique, so the k smallest keys ARE
        the (distance, id)-ordered top-k) -> one batched ``torch.topk`` per chunk.  No per-query sort, no host round trip."""
        from ..._capi import LAYOUT_BMK, LAYOUT_TILED  # noqa: F401

        kind, xq = scan_in if scan_in is not None else self.pq_codec.scan_inputs(q)
        lut = ops.lut_build(xq, self.pq_codec.codebooks_dev, kind, LAYOUT_BMK)
        codes = self._plain_codes(N)
        dev = q.device
        vb = self._unpack_bits(valid, N)
        kk = min(k, N)
        B = q.shape[0]
        chunk = max(1, min(B, (1 << 26) // max(N, 1)))  # <= 64M keys (512 MB) + their f32 sums per chunk (the flat index: half)
        rows = torch.arange(N, device=dev, dtype=torch.int64)
        inf = torch.tensor(float('inf'), device=dev)
        key_none = torch.tensor(torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
        ds, is_ = [], []
        for b0 in range(0, B, chunk):
            nb = min(chunk, B - b0)
            dist = torch.empty((nb, N), dtype=torch.float32, device=dev)
            for j in range(nb):
                ops.adc_dist(lut[b0 + j], codes, out=dist[j])
            # -0.0 -> +0.0 before keying: equal VALUES tie-break by id, what the scan kernels' lists do with ADC sums (the flat
            # index's exact distances keep key(-0.0) < key(+0.0): FlatGpuIndex._keyed_topk)
            keys = (float_order_key(dist + 0.0) << 32) | rows[None, :]
            keys = torch.where(vb[None, :], keys, key_none)  # deleted / never-written rows: behind every real row, NaN ones included
            top = torch.topk(keys, kk, dim=1, largest=False, sorted=True).values
            none = top == key_none
            # (a real row at +inf keeps its id here; the flat index blanks it, as its k <= 64 kernel does)
            ds.append(torch.where(none, inf, float_from_key(top >> 32)))
            is_.append(torch.where(none, torch.full_like(top, -1), top & 0xFFFFFFFF))
        d, i = pad_to_k(torch.cat(ds), torch.cat(is_), k)
        if self.metric == Metric.EUCLIDEAN:
            d = torch.sqrt(d)
        return d, i

    @staticmethod
    def _topk_rows_any(values: torch.Tensor, k: int):
        """Row-wise k smallest with positions, (value, position) ascending: the wave kernel for k <= 64, a stable device
        sort beyond (a large `limit` must not be cut to 64 silently)."""
        if k <= 64:
            return ops.topk_rows(values, k)
        sd, si = torch.sort(values, dim=1, stable=True)
        sd, si = sd[:, :k], si[:, :k]
        return sd, torch.where(torch.isinf(sd), torch.full_like(si, -1), si)

    def _search_rerank(self, q, k, valid, N, rerank_k, scan_in=None, filtered=False):
        B = q.shape[0]
        # candidates per row slice: 16 where the byte-table kernel generates them (M = 16: 8 slices x 16 keys = 128 per query
        # at 1024 queries; its lists hold 16 keys), 64 otherwise (u16-table kernels)
        byte_tables = self.M == 16 and self.code_bytes == 1 and self.Ks <= 256 and self.scan_kernel != 'u16 tables'
        asked = rerank_k or getattr(self, 'rerank_k', None)
        rk = max(1, min(64, int(asked or (16 if byte_tables else 64))))
        plan = scan_plan(N, self.M, self.Ks, self.code_bytes, B, rk)
        if not asked:
            # The pool is n_slices * rk rows per query, and a small table or a huge batch plans 1-4 slices: the default must
            # still hand the re-rank MORE than k candidates (k of k re-ranks nothing, fewer than k returns padding) -- at
            # least max(64, 4 k) where the table has them.  Beyond the byte-table lists' 16 keys the u16-table generator
            # (up to 64 keys per slice) takes over: scan_plan picks it from rk.
            want = max(64, 4 * k)
            for _ in range(2):  # (the tile width, hence n_slices, can change with the generator)
                if plan.n_slices * rk >= want or rk >= 64:
                    break
                rk = min(64, -(-want // max(plan.n_slices, 1)))
                plan = scan_plan(N, self.M, self.Ks, self.code_bytes, B, rk)
        from ..._capi import LAYOUT_BMK, LAYOUT_TILED

        kind, xq = scan_in if scan_in is not None else self.pq_codec.scan_inputs(q)
        # (the global pool holds at most 64 rows: a larger `limit` takes the slice pool, n_slices * rk rows -- never 64 real rows
        # plus padding; a filtered call -- `valid` is the caller's mask, not the table's own bitmap -- keeps its candidate counts out
        # of the table's kernel-choice state, as search_batch does)
        if getattr(self, 'rerank_pool', 'slices') == 'global' and k <= 64:
            # Pool = the GLOBAL ADC top-R (R <= 64) of the shared-bound search -- since round 5 the byte-table kernel serves it
            # (64-key lists) -- instead of the union of per-slice top-16 lists: 50 rows that are the 50 best by ADC distance
            # against 128 of which only the 16 best are guaranteed.  One C call, then the exact re-score as below.
            R = max(min(k, 64), min(64, int(asked or 50)))
            _, cand = ops.pq_search_topk(kind, xq, self.pq_codec.codebooks_dev, self._codes, R, self.M, self.Ks, valid_bits=valid,
                                         n_rows=N, codes_layout=self._layout(), workspace=self._ws,
                                         state=None if filtered else self.scan_state)
        else:
            # (round 6) tables + candidate generator in one C call; M = 16 / L2: through the plain search's ONE preparation launch
            _, cand = ops.pq_search_candidates(kind, xq, self.pq_codec.codebooks_dev, self._codes, rk, self.M, self.Ks, valid_bits=valid,
                                               n_rows=N, codes_layout=self._layout(), workspace=self._ws)
        if k <= 64:  # (round 6) exact distances + top-k + ids + sqrt in one launch, a wave per query; same numbers as below
            return ops.rerank_topk(int(self.metric), q, self._vectors, cand, k, sqrt=self.metric == Metric.EUCLIDEAN)
        exact = ops.exact_gather_dist(int(self.metric), q, self._vectors, cand)  # [B, R]
        kk = min(k, cand.shape[1])
        d, pos = self._topk_rows_any(exact, kk)
        return ranked_answer(cand, d, pos, k, sqrt=self.metric == Metric.EUCLIDEAN)

    # ------------------------------------------------------------------ persistence (envelope: row_store.py)
    def _dump_state(self, N):
        """Codes are saved in the PLAIN (reference) layout."""
        return {'metric': int(self.metric),
                'codes': ops.codes_to_numpy(self._plain_codes(N)) if N else np.zeros((0, self.M), self.pq_codec.code_dtype),
                'vectors': self._vectors[:N].cpu().numpy() if self._vectors is not None else None}

    def _load_state(self, state, N):
        if N:
            codes = self._to_dev(state['codes'])
            if self._layout() == CODES_SKEWED:
                ops.codes_skew(codes, ids=None, id_base=0, out=self._codes)
            else:
                self._codes[:N] = codes
            if self._vectors is not None and state['vectors'] is not None:
                self._vectors[:N] = self._to_dev(state['vectors'])
        if self._scan_state is not None:
            self._scan_state.reset()  # (another table: what was measured no longer applies)
