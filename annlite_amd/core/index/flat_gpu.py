"""``FlatGpuIndex`` -- exact search over un-quantised float vectors on one MI355X: what the reference builds for
``AnnLite(n_dim)`` without ``n_subvectors`` (``HnswIndex`` on float vectors, annlite/core/index/hnsw/index.py:139-167; brute-force
form ``FlatIndex``, annlite/core/index/flat_index.py:15-39: ``cdist`` + ``top_k``).

Same plug-in surface as ``PQFlatGpuIndex`` (``add_with_ids`` / ``update_with_ids`` / ``delete`` / ``reset`` / ``search`` /
``search_batch`` / ``dump`` / ``load``, capacity growing by ``expand_step_size``, device storage allocated on first use): both are
``RowStoreIndex`` (row_store.py) with columns of their own -- this module holds what is the float index's alone.  HBM
holds ``f32 [capacity, D]`` vectors, ``f32 [capacity]`` squared norms (written by a kernel at add / update) and the validity
bitmap.  A search is ONE C call (``annlite_flat_search_topk``): an f32 MFMA contraction filters the table
against a per-query bound with a proven slack, a wave per query re-scores the rows that passed in ``annlite_rerank_topk``'s
arithmetic.  The answer is exact in that arithmetic: a stored vector searched with itself comes back at distance 0.0.

Where it is slow (and still exact): the filter's slack is relative to ``|x|^2 + |q|^2``, not to the distance.  Data with a large
common offset (every coordinate near 1000) makes it exceed every distance: all rows pass, the lists overflow and each query is
answered by one wave over ALL rows (``last_overflowed`` counts them).  ``flat_filter='bf16x3'`` is the filter for such data: it
contracts the rows minus a fixed centre (``centre='mean'``: the mean of the first batch added), carried as two bf16 numbers each, on
three bf16 MFMAs, and its slack is relative to ``|x - centre|^2 + |q - centre|^2``; the answer keeps its bits (DESIGN.md section 3.6,
"split filter").  The all-rows route also serves NaN / infinite queries and searches restricted (``indices=``, deletes) to fewer
than about k rows in 4096, under either filter.

``dtype=np.float16`` stores the rows in half precision: ``f16 [capacity, D]``, half the bytes in HBM.  Rows are pre-processed as always
(COSINE: normalised in f32) and rounded to f16 once, to nearest even, when they are written; queries stay f32.  The answer is, bit
for bit, the f32 index's over the rounded rows widened back to f32: the exact stage keeps its arithmetic, and an f16 row is an exact
MFMA operand, so the filter (``'f16x2'``: the query carried as two f16 numbers, two f16 MFMAs) needs no centre and no split of the rows
("f16 rows").  A value beyond the f16 range (65504) is stored as an infinity and behaves as the f32 index
holding that infinity does.  There is no centre: a common offset destroys f16 data before any filter sees it (1000.37 is stored as
1000.5) -- centre such data before adding it.

``dtype=np.int8`` stores the rows as int8 codes: ``int8 [capacity, D]``, a quarter of the bytes.  A coordinate ``x`` (pre-processed as
always: COSINE normalises in f32 first) is stored as ``c = clamp(rne(x / s), -127, 127)`` and stands for the value ``s * c``; the scale
``s = int8_scale`` is a power of two in ``[2**-24, 2**24]``, so ``x / s`` and ``s * c`` are exact in f32 (default ``1.0`` for EUCLIDEAN and
INNER_PRODUCT -- int8 embeddings as given -- and ``2**-7`` for COSINE, whose coordinates lie in [-1, 1]).  Rounding is to nearest even;
values beyond ``+-127 s``, the infinities included, saturate; a NaN coordinate is stored as 0; -128 is never stored.  Queries stay f32.
The answer is, bit for bit, what the f32 index returns when it holds the rows ``s * c``: the exact stage keeps its arithmetic on the
widened values, and the filter (``'i8x3'``: the query rounded to a 21-bit integer and carried as three int8 digits, three i8 MFMAs
into integer accumulators) contracts without any rounding at all ("int8 rows").  No centre, as for f16.
"""
import math
from functools import partial
from pathlib import Path
from typing import Callable, NamedTuple, Optional, Tuple, Union

import numpy as np
import torch

from ... import ops
from ...enums import Metric
from .base import str2dtype
from .row_store import RowStoreIndex, empty_answer, float_from_key, float_order_key, group_chunks, like_input, pad_to_k


def flat_slack_constants(metric: Metric, dim: int) -> Tuple[np.float32, np.float32]:
    """``(c_rel, c_abs)`` of the filter's slack ``c_rel * fl(|x|^2 + |q|^2) + c_abs`` -- the numbers the library hands its filter
    kernel (``annlite_flat_slack``; derivation: DESIGN.md section 3.6)."""
    return ops.flat_slack(int(Metric(metric)), dim)


def flat_split_slack_constants(metric: Metric, dim: int) -> Tuple[np.float32, np.float32]:
    """``(c_rel, c_abs)`` of the split filter (``flat_filter='bf16x3'``), where the norms are those of the centred values
    (``annlite_flat_split_slack``; derivation: DESIGN.md section 3.6, "split filter")."""
    return ops.flat_split_slack(int(Metric(metric)), dim)


def flat_f16_slack_constants(metric: Metric, dim: int) -> Tuple[np.float32, np.float32]:
    """``(c_rel, c_abs)`` of the f16 filter (``dtype=np.float16``); its slack has a third, per-query term the library computes,
    ``1.001 * 2^-13 * sum |q_j|`` (``annlite_flat_f16_slack``; derivation: DESIGN.md section 3.6, "f16 rows")."""
    return ops.flat_f16_slack(int(Metric(metric)), dim)


def flat_i8_slack_constants(metric: Metric, dim: int) -> Tuple[np.float32, np.float32]:
    """``(c_rel, c_abs)`` of the int8 filter (``dtype=np.int8``); its slack has a third, per-query term the library computes,
    ``1.001 * 127 * dim * 2^-e`` with ``2^e`` the query's power of two (``annlite_flat_i8_slack``; derivation:
    DESIGN.md section 3.6, "int8 rows")."""
    return ops.flat_i8_slack(int(Metric(metric)), dim)


def row_kind(dtype) -> str:
    """How a ``dtype=`` argument (any spelling ``base.str2dtype`` takes) has ``FlatGpuIndex`` store its rows: ``'f16'``, ``'i8'`` or
    -- every other dtype -- ``'f32'``."""
    try:
        dt = np.dtype(str2dtype(dtype) if isinstance(dtype, str) else dtype)
    except TypeError:
        return 'f32'
    return 'f16' if dt == np.float16 else 'i8' if dt == np.int8 else 'f32'


def is_f16(dtype) -> bool:
    """whether a ``dtype=`` argument selects half-precision rows"""
    return row_kind(dtype) == 'f16'


def is_i8(dtype) -> bool:
    """whether a ``dtype=`` argument selects int8 rows"""
    return row_kind(dtype) == 'i8'


I8_SCALE_LOG2_RANGE = (-24, 24)


def check_i8_scale(scale) -> float:
    """``int8_scale`` as a float: a positive power of two in ``[2**-24, 2**24]``, else ``ValueError``"""
    try:
        value = float(scale)
        mant, exp = math.frexp(value)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f'int8_scale={scale!r}: a power of two in [2**-24, 2**24]') from None
    if not (value > 0 and mant == 0.5 and I8_SCALE_LOG2_RANGE[0] <= exp - 1 <= I8_SCALE_LOG2_RANGE[1]):
        raise ValueError(f'int8_scale={scale!r}: a power of two in [2**-24, 2**24]')
    return value


def quantise_i8(x: torch.Tensor, scale: float) -> torch.Tensor:
    """f32 ``x`` -> the int8 codes ``clamp(rne(x / scale), -127, 127)``, NaN -> 0 (``x / scale`` is exact: the scale is a power of
    two; ``torch.round`` rounds halves to even)."""
    t = torch.nan_to_num(x.to(torch.float32) * (1.0 / scale), nan=0.0, posinf=127.0, neginf=-127.0)
    return torch.round(t).clamp_(-127.0, 127.0).to(torch.int8)


def _rows_f32(x: torch.Tensor) -> torch.Tensor:
    return x


def _rows_f16(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.float16)


class _RowKind(NamedTuple):
    """What serves the rows of one store -- f32, f16 or int8 --, with the scale of an int8 store bound in: resolved once per index."""
    dtype: torch.dtype
    encode: Callable       # f32 rows -> the stored values (f16: rounded once, to nearest even; int8: quantise_i8)
    norms: Callable        # ops.flat_row_norms(vectors, ids=, n=, out=) of the store
    gather_dist: Callable  # ops.exact_gather_dist(metric, queries, vectors, cand) of the store
    topk: Callable         # ops.flat_search_topk(metric, queries, vectors, norms, k, ...) of the store and its filter
    tag: str               # that filter's name in ``last_flat_filter``
    stage: Callable        # one filter stage, (metric, queries, vectors, norms, bounds, ...) -> (cand, count, ...): the k > 64 search


def _resolve_row_kind(kind: str, i8_scale: Optional[float], workspace) -> _RowKind:
    if kind == 'i8':
        s = i8_scale
        return _RowKind(torch.int8, partial(quantise_i8, scale=s), partial(ops.flat_row_norms_i8, scale=s),
                       partial(ops.exact_gather_dist_i8, scale=s), partial(ops.flat_search_topk_i8, scale=s), 'i8x3',
                       partial(ops.flat_filter_i8, scale=s, workspace=workspace))
    if kind == 'f16':
        return _RowKind(torch.float16, _rows_f16, ops.flat_row_norms_f16, ops.exact_gather_dist_f16,
                       ops.flat_search_topk_f16, 'f16x2', partial(ops.flat_filter_f16, workspace=workspace))
    # (f32 rows have a second filter, 'bf16x3': ``flat_filter`` is read at every search, by search_batch)
    return _RowKind(torch.float32, _rows_f32, ops.flat_row_norms, ops.exact_gather_dist, ops.flat_search_topk, 'f32', ops.flat_filter)


class FlatGpuIndex(RowStoreIndex):
    """
    :param dtype: ``np.float32`` (default), ``np.float16`` or ``np.int8``: how the rows are stored (module docstring).  ``np.float16``
        and ``np.int8`` take neither ``flat_filter='bf16x3'`` nor a ``centre`` and need ``dim <= 32768``; any other dtype stores f32.
    :param int8_scale: with ``dtype=np.int8`` only: the value of one code step, a power of two in ``[2**-24, 2**24]``.  ``None``
        (default): ``1.0`` for EUCLIDEAN and INNER_PRODUCT, ``2**-7`` for COSINE.  ``int8_scale_`` reads the one in use.
    :param flat_filter: ``'f32'`` (default): the f32 MFMA filter.  ``'bf16x3'``: the split-bf16 filter over centred rows -- the same
        answer bit for bit, a slack that does not grow with a common offset of the data, ``dim <= 32768``.  Searches with
        ``limit > 64`` keep the f32 filter under either value: offset data stays slow there.  ``'f16x2'``: the filter over f16 rows --
        what ``dtype=np.float16`` runs (and reports here), at every ``limit``; with f32 rows it is an error.  ``'i8x3'``: the same
        for ``dtype=np.int8``.
    :param centre: what ``'bf16x3'`` subtracts from rows and queries before it splits them, EUCLIDEAN only -- INNER_PRODUCT and COSINE
        are not invariant under a shift and run the split filter on the values themselves.  ``'mean'`` (default): the f32 mean of the
        first ``add_with_ids`` batch, frozen until ``reset()``; an array ``[dim]``: that point; ``None``: no centring.  Any centre gives
        the exact answer; it only moves the slack (a NaN or infinite one -- the mean of a first batch that holds such a value --
        lets every row pass: every query then takes the all-rows route).  ``centre_`` reads the one in use.
    :param filter_route: how a search restricted to a subset -- ``indices`` (offsets or a ``RowMask``) or deleted rows -- scans.
        ``'mask'`` (default): the whole table, a row's bit tested once its score exists: a row that fails costs what one that passes
        does.  ``'rows'``: the selection is compacted into an ascending list of offsets (``annlite_bitmap_rows``; 4 bytes per row of
        capacity, kept by the index) and the search -- first sample, filter stages, overflow route -- runs over that list: the work
        follows the number of selected rows ("selected rows").  Reading that number is one host read per
        search.  At most 4096 selected rows are answered by exact sums over the list (no filter runs), none by the empty answer.
        ``'auto'``: ``'rows'`` where the selection holds at most ``ROWS_MAX_FRACTION`` of the rows, else ``'mask'``
        (``choose_filter_route``).  The answer is the same bit for bit under every value.  A search with no ``indices`` and no
        deleted rows has nothing to compact, and ``limit > 64`` keeps the masked ``_search_large_k``: both stay ``'mask'`` under every
        value.  ``search_batch`` takes the keyword per call; ``last_filter_route`` reports ``'mask'`` / ``'rows'`` for the last search
        (``None``: none yet, or an empty index or batch), and ``last_overflowed`` counts the queries sent to exact sums over all rows
        of whatever set was scanned.
    """
    FORMAT = 'annlite_amd.FlatGpuIndex/1'
    STATE_KEYS = ('dim', 'metric')
    FLAT_FILTERS = ('f32', 'bf16x3', 'f16x2', 'i8x3')
    SPLIT_MAX_DIM = 32768    # (annlite_flat_split_slack: the range of the slack's derivation)
    FILTER_MIN_ROWS = 4097   # (kFlatSample + 1 in flat.hip: smaller tables are answered by exact sums, no filter runs)
    FILTER_ROUTES = ('mask', 'rows', 'auto')
    ROWS_MAX_FRACTION = 0.5  # (measured: DESIGN.md section 3.6, "selected rows")

    def __init__(self, dim: int, dtype: np.dtype = np.float32, metric: Metric = Metric.COSINE,
                 index_file: Optional[Union[str, Path]] = None, flat_filter: str = 'f32', centre='mean', int8_scale=None,
                 filter_route: str = 'mask', **kwargs):
        self.filter_route = self._check_filter_route(filter_route)
        self.last_filter_route = None  # 'mask' / 'rows': how the last search_batch scanned; None: it scanned nothing
        self._sel_rows = None          # i32 [capacity]: the compacted selection of the last 'rows' search
        self._rows_ws = ops.ScanWorkspace()
        if flat_filter not in self.FLAT_FILTERS:
            raise ValueError(f"flat_filter={flat_filter!r}: 'f32' (the f32 MFMA filter), 'bf16x3' (the split-bf16 filter over centred rows) "
                             "or, with dtype=np.float16, 'f16x2', with dtype=np.int8, 'i8x3'")
        kind = row_kind(dtype)
        self._f16, self._i8 = kind == 'f16', kind == 'i8'
        self._i8_scale = None
        if self._i8:
            if flat_filter in ('bf16x3', 'f16x2'):
                raise ValueError(f"flat_filter={flat_filter!r} is not a filter over int8 rows: dtype=np.int8 runs 'i8x3'")
            if not (isinstance(centre, str) and centre == 'mean'):
                raise ValueError(f'centre={centre!r} with dtype=np.int8: int8 rows have no centre (centre the data before adding it)')
            if dim > self.SPLIT_MAX_DIM:
                raise ValueError(f'dtype=np.int8 takes dim <= {self.SPLIT_MAX_DIM}')
            self._i8_scale = check_i8_scale((2.0 ** -7 if Metric(metric) == Metric.COSINE else 1.0) if int8_scale is None else int8_scale)
            flat_filter = 'i8x3'
        elif int8_scale is not None:
            raise ValueError(f'int8_scale={int8_scale!r} is the scale of int8 rows: pass dtype=np.int8')
        elif flat_filter == 'i8x3':
            raise ValueError("flat_filter='i8x3' is the filter over int8 rows: pass dtype=np.int8")
        if self._f16:
            if flat_filter == 'bf16x3':
                raise ValueError("flat_filter='bf16x3' splits f32 rows: dtype=np.float16 runs 'f16x2'")
            if not (isinstance(centre, str) and centre == 'mean'):
                raise ValueError(f'centre={centre!r} with dtype=np.float16: f16 rows have no centre (centre the data before adding it)')
            if dim > self.SPLIT_MAX_DIM:
                raise ValueError(f'dtype=np.float16 takes dim <= {self.SPLIT_MAX_DIM}')
            flat_filter = 'f16x2'
        elif flat_filter == 'f16x2':
            raise ValueError("flat_filter='f16x2' is the filter over f16 rows: pass dtype=np.float16")
        if isinstance(centre, str) and centre != 'mean':
            raise ValueError(f"centre={centre!r}: 'mean', None or an array of {dim} coordinates")
        if centre is not None and not isinstance(centre, str):
            centre = np.array(centre.cpu() if isinstance(centre, torch.Tensor) else centre, dtype=np.float32)
            if centre.shape != (dim,):
                raise ValueError(f'centre has shape {centre.shape}: ({dim},) expected')
        if flat_filter == 'bf16x3' and dim > self.SPLIT_MAX_DIM:
            raise ValueError(f"flat_filter='bf16x3' takes dim <= {self.SPLIT_MAX_DIM}")
        self.flat_filter = flat_filter
        self.centre = centre
        self.last_flat_filter = None  # 'f32' / 'bf16x3' / 'f16x2' / 'i8x3': the filter of the last search_batch; None: it ran none
        self._centre_dev = None
        self._centred = flat_filter == 'bf16x3' and Metric(metric) == Metric.EUCLIDEAN and centre is not None
        self._ws = ops.ScanWorkspace()
        self._kind = _resolve_row_kind(kind, self._i8_scale, self._ws)
        super().__init__(dim, dtype=dtype, metric=metric, **kwargs)
        self._overflowed = 0  # (of the last search_batch; None: ask the library's workspace)
        if index_file:
            self.load(index_file)

    @property
    def int8_scale_(self) -> Optional[float]:
        """The value of one code step of an int8 row store; None for the other dtypes."""
        return self._i8_scale

    # ------------------------------------------------------------------ the split filter's centre
    @property
    def centre_(self) -> Optional[np.ndarray]:
        """The centre the split filter subtracts, f32 ``[dim]``; None: none (the f32 filter, another metric, ``centre=None``, or
        ``'mean'`` before the first rows arrived)."""
        return None if self._centre_dev is None else self._centre_dev.cpu().numpy()

    def _fix_centre(self, rows: torch.Tensor, stored=None):
        """Settle the centre once: the constructor's array, else the one an index file carried, else the f32 mean of ``rows``."""
        if not self._centred or self._centre_dev is not None:
            return
        if not isinstance(self.centre, str):
            self._centre_dev = self._to_dev(self.centre, torch.float32).contiguous()
        elif stored is not None:
            self._centre_dev = self._to_dev(np.asarray(stored, dtype=np.float32).reshape(self.dim), torch.float32).contiguous()
        else:
            self._centre_dev = rows.to(torch.float32).mean(dim=0).contiguous()

    def reset(self, capacity: Optional[int] = None):
        super().reset(capacity=capacity)
        self._centre_dev = None

    def _alloc(self, capacity: int):
        super()._alloc(capacity)
        self._sel_rows = None  # (made at the new capacity by the next 'rows' search)

    # ------------------------------------------------------------------ storage (row_store.py)
    def _columns(self):
        """``_cnorms``: the norms of the centred rows, kept only where the split filter has a centre (it reads ``_norms`` otherwise)"""
        return {'_vectors': ((self.dim,), self._kind.dtype), '_norms': ((), torch.float32),
                '_cnorms': ((), torch.float32) if self._centred else None}

    def _write_rows(self, x, ids):
        # flat_index.py:41-50 `_data[ids] = x`; f16: rounded once, to nearest even, beyond the f16 range an infinity; int8: rounded once, to
        # nearest even, saturating at +-127, NaN: 0
        self._vectors[ids] = self._kind.encode(x)
        self._kind.norms(self._vectors, ids=ids, out=self._norms)
        if self._centred:
            self._fix_centre(x)
            ops.flat_centred_norms(self._vectors, self._centre_dev, ids=ids, out=self._cnorms)

    def _dump_state(self, N):
        """vectors as stored (normalised for COSINE; in the index's dtype); norms are recomputed on load.  ``centre`` (optional key):
        the split filter's; ``int8_scale`` (optional key): what one step of int8 ``vectors`` stands for"""
        state = {'vectors': self._vectors[:N].cpu().numpy()}
        if self._i8:
            state['int8_scale'] = float(self._i8_scale)
        if self._centre_dev is not None:
            state['centre'] = self.centre_
        return state

    def _load_state(self, state, N):
        self._centre_dev = None
        if N:
            # (a file of another dtype is converted: f32 into an f16 index rounds, f16 into an f32 index widens, floats into an int8
            # index are quantised with the index's scale, int8 codes into a float index are widened with the file's)
            stored = self._to_dev(state['vectors'])
            if stored.dtype == torch.int8:
                file_scale = check_i8_scale(state.get('int8_scale', 1.0))
                if self._i8 and file_scale != self._i8_scale:
                    raise ValueError(f'the file holds int8 rows of int8_scale={file_scale!r}, this index stores int8_scale={self._i8_scale!r}: '
                                     'codes of one scale are not codes of another (load into a float index, or construct with the '
                                     "file's scale)")
                if not self._i8:
                    stored = stored.to(torch.float32) * file_scale  # (exact)
            else:
                stored = self._kind.encode(stored)
            self._vectors[:N] = stored.to(self._vectors.dtype)
            self._kind.norms(self._vectors, n=N, out=self._norms)
            if self._centred:  # (a file without the key -- an older one, an f32 index's: the mean of the rows it holds)
                self._fix_centre(self._vectors[:N], stored=state.get('centre'))
                ops.flat_centred_norms(self._vectors, self._centre_dev, n=N, out=self._cnorms)

    # ------------------------------------------------------------------ search
    @property
    def last_overflowed(self) -> int:
        """Queries of the last ``search_batch`` whose candidate list overflowed: they were answered by exact sums over all rows
        -- the slower route.  0 after a search that ran no filter (empty index, empty batch)."""
        if self._overflowed is None:
            self._overflowed = ops.flat_overflow_count(self._ws)
        return self._overflowed

    @classmethod
    def _check_filter_route(cls, route) -> str:
        if route not in cls.FILTER_ROUTES:
            raise ValueError(f"filter_route={route!r}: 'mask' (scan the table, test a row's bit), 'rows' (compact the selection, scan "
                             "only its rows) or 'auto' (by the selection's share of the rows)")
        return route

    def choose_filter_route(self, n_sel: Optional[int], n_rows: int, k: int, route: Optional[str] = None) -> str:
        """``'mask'`` or ``'rows'`` for a search of ``limit`` ``k`` whose selection holds ``n_sel`` of ``n_rows`` rows (``None``: nothing
        to compact -- no ``indices``, no deleted rows) under ``route`` (default: the index's ``filter_route``).  Pure: no device work."""
        route = self.filter_route if route is None else self._check_filter_route(route)
        if route == 'mask' or n_sel is None or k > 64:
            return 'mask'
        if route == 'rows':
            return 'rows'
        return 'rows' if n_sel <= self.ROWS_MAX_FRACTION * n_rows else 'mask'

    def _filter_operands(self):
        """``(tag, norms, centre)`` of the filter a ``limit <= 64`` search runs: the row kind's own or, over f32 rows with
        ``flat_filter='bf16x3'``, the split filter with the centred norms and the centre where the index keeps one (k > 64: the f32 filter)."""
        tag, norms, centre = self._kind.tag, self._norms, None
        if self.flat_filter == 'bf16x3' and tag == 'f32':
            tag = 'bf16x3'
            if self._centred:
                norms, centre = self._cnorms, self._centre_dev
        return tag, norms, centre

    def _search_rows(self, q, k: int, valid, N: int, route: str):
        """The ``'rows'`` route of a k <= 64 search over the rows set in ``valid``; None where ``'auto'`` decides for the mask."""
        if self._sel_rows is None or self._sel_rows.numel() < self._capacity:
            self._sel_rows = torch.empty((max(self._capacity, N),), dtype=torch.int32, device=q.device)
        _, n_sel = ops.bitmap_rows(valid, n_rows=N, out=self._sel_rows, workspace=self._rows_ws)  # (the one host read)
        if self.choose_filter_route(n_sel, N, k, route) != 'rows':
            return None
        self.last_filter_route = 'rows'
        if n_sel == 0:
            return empty_answer(q.shape[0], k, q.device)
        tag, norms, centre = self._filter_operands()
        d, i = ops.flat_search_topk_rows(tag, int(self.metric), q, self._vectors, norms, self._sel_rows, k, n_sel=n_sel, n_rows=N, centre=centre,
                                         scale=self._i8_scale or 1.0, sqrt=self.metric == Metric.EUCLIDEAN, workspace=self._ws)
        self._overflowed = None
        self.last_flat_filter = tag if n_sel >= self.FILTER_MIN_ROWS else None
        return d, i

    def search_batch(self, x, limit: int = 10, indices=None, filter_route: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """All queries of ``x`` [B, D] in one call.  ``(dists f32 [B, k], ids i64 [B, k])`` ascending by (distance, id), NaN
        distances last; missing -> (+inf, -1).  numpy in gives numpy out, device tensors stay on the device.  ``filter_route``: this
        call's, else the constructor's (class docstring); ``limit > 64`` keeps the masked search under every value."""
        route = self.filter_route if filter_route is None else self._check_filter_route(filter_route)
        is_np = not isinstance(x, torch.Tensor)
        q = self._pre(x)
        B = q.shape[0]
        k = int(limit)
        assert k >= 1
        N = self._n_rows
        dev = q.device
        self._overflowed = 0
        self.last_flat_filter = None
        self.last_filter_route = None
        if N == 0 or B == 0:
            d, i = empty_answer(B, k, dev)
        else:
            valid = self._valid if indices is None else self._filter_bits(indices)
            answer = None
            # (something to compact: a subset was asked for, or rows below the highest one are not valid)
            if k <= 64 and route != 'mask' and (indices is not None or self._size < N):
                answer = self._search_rows(q, k, valid, N, route)
            if answer is not None:
                d, i = answer
                return like_input(is_np, d, i)
            self.last_filter_route = 'mask'
            if k <= 64:  # hnsw/index.py:164-165
                tag, norms, centre = self._filter_operands()
                topk = partial(ops.flat_search_topk_split, centre=centre) if tag == 'bf16x3' else self._kind.topk
                d, i = topk(int(self.metric), q, self._vectors, norms, k, valid_bits=valid, n_rows=N, sqrt=self.metric == Metric.EUCLIDEAN,
                            workspace=self._ws)
                self._overflowed = None  # (read from the workspace when asked for: it costs a synchronisation)
                self.last_flat_filter = tag if N >= self.FILTER_MIN_ROWS else None
            else:
                d, i = self._search_large_k(q, k, valid, N)
        return like_input(is_np, d, i)

    def search_batch_grouped(self, x, limit: int = 10, selections=(), group_of=()):
        """``RowStoreIndex.search_batch_grouped`` in ONE launch for ``limit <= 64`` on a non-empty index (``last_filter_batch =
        'grouped'``): the selections become a ``[G, n_words]`` mask tensor (``_filter_bits`` each, None: the live bitmap) and the
        search is ``annlite_flat_search_topk_grouped`` with the index's row kind and filter -- full query tiles, one first sample per
        query, a bit test per pair that passed the bound ("a filter per query").  Row b is, bit for bit, what
        ``search_batch`` answers query b under its selection.  More than ``MAX_FILTER_GROUPS`` groups with queries: the queries are split
        by group into several such launches.  ``limit > 64`` and an empty index take the looping form.  ``last_flat_filter`` and
        ``last_overflowed`` as after ``search_batch``; the scan is over the table (``last_filter_route = 'mask'``)."""
        k = int(limit)
        assert k >= 1
        if k > 64 or self._n_rows == 0:
            return super().search_batch_grouped(x, limit=limit, selections=selections, group_of=group_of)
        is_np = not isinstance(x, torch.Tensor)
        q = self._pre(x)
        B, N, dev = q.shape[0], self._n_rows, q.device
        group = self._check_groups(B, selections, group_of)
        self._overflowed = 0
        self.last_flat_filter = None
        self.last_filter_route = None
        self.last_filter_batch = 'grouped'
        if B == 0:
            return like_input(is_np, *empty_answer(B, k, dev))
        tag, norms, centre = self._filter_operands()
        d, i = None, None
        for groups, queries, local in group_chunks(group, self.MAX_FILTER_GROUPS):
            masks = torch.stack([self._valid if selections[int(g)] is None else self._filter_bits(selections[int(g)]) for g in groups]).contiguous()
            at, qs = None, q
            if queries is not None:
                at = torch.as_tensor(queries, device=dev)
                qs = q[at].contiguous()
                if d is None:
                    d, i = empty_answer(B, k, dev)
            cd, ci = ops.flat_search_topk_grouped(tag, int(self.metric), qs, self._vectors, norms, masks,
                                                  torch.as_tensor(local.astype(np.int32), device=dev), k, valid_bits=self._valid, n_rows=N,
                                                  centre=centre, scale=self._i8_scale or 1.0, sqrt=self.metric == Metric.EUCLIDEAN,
                                                  workspace=self._ws)
            if at is None:
                d, i = cd, ci
                self._overflowed = None  # (read from the workspace when asked for: it costs a synchronisation)
            else:
                d[at], i[at] = cd, ci
                self._overflowed += ops.flat_overflow_count(self._ws)  # (the next launch takes the counter over)
        self.last_filter_route = 'mask'
        self.last_flat_filter = tag if N >= self.FILTER_MIN_ROWS else None
        return like_input(is_np, d, i)

    def _gather_dist(self, q, cand):
        return self._kind.gather_dist(int(self.metric), q, self._vectors, cand)

    def _keyed_topk(self, q, cand, ok, kk):
        """The ``kk`` nearest of each query's candidates ``cand`` i64 [b, R] (``ok``: which entries count) by exact distance
        (``annlite_exact_gather_dist``: a wave per pair, the numbers of the k <= 64 path): i64 keys -- order-preserving bits of the
        distance << 32 | row id, unique, so the smallest keys ARE the (distance, id) order, NaN last -- and one ``torch.topk``."""
        dist = self._gather_dist(q, cand)
        # (no `+ 0.0` before keying, unlike PQFlatGpuIndex._search_large_k: key(-0.0) < key(+0.0) is annlite_rerank_topk's order,
        # whose numbers this path returns)
        key_none = torch.iinfo(torch.int64).max
        keys = (float_order_key(dist) << 32) | cand.clamp(min=0)
        keys = torch.where(ok, keys, torch.full_like(keys, key_none))
        top = torch.topk(keys, kk, dim=1, largest=False, sorted=True).values
        none = top == key_none
        sd = float_from_key(top >> 32)
        sd = torch.where(none, torch.full_like(sd, float('inf')), sd)
        # (+inf: a missing place, as annlite_rerank_topk blanks it; the PQ index's large-k path returns such a row's id)
        si = torch.where(none | (sd == float('inf')), torch.full_like(top, -1), top & 0xFFFFFFFF)
        return sd, si

    def _all_rows_topk(self, q, kk, vb, N):
        """``_keyed_topk`` over every row, in query chunks: the route of small tables and of overflowed lists."""
        rows = torch.arange(N, device=q.device, dtype=torch.int64)
        chunk = max(1, min(q.shape[0], (1 << 25) // max(N, 1)))  # (32M keys: half the PQ path's budget, next to them the gathered f32 rows)
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
        vb = self._unpack_bits(valid, N)
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
                ds = self._gather_dist(q[b0:b0 + nb].contiguous(), sample[None, :].expand(nb, -1).contiguous())
                ds = torch.where(s_ok[None, :], torch.nan_to_num(ds, nan=float('inf'), posinf=float('inf'), neginf=float('-inf')),
                                 torch.full_like(ds, float('inf')))
                bounds.append(torch.topk(ds, kk, dim=1, largest=False).values[:, kk - 1] if sample.numel() >= kk
                              else torch.full((nb,), float('inf'), device=dev))
            bound = torch.cat(bounds).contiguous()  # (+inf -- fewer than k valid sampled rows, NaN distances -- passes everything)
            cand32, count = self._kind.stage(int(self.metric), q, self._vectors, self._norms, bound, valid_bits=valid, n_rows=N)[:2]
            self.last_flat_filter = self._kind.tag
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
        d, i = pad_to_k(d, i, k)
        if self.metric == Metric.EUCLIDEAN:
            d = torch.sqrt(d)
        return d, i
