"""``AnnLite`` facade -- the reference's public API (annlite/index.py:26-973) over the MI355X
PQ/ADC hot path.

Kept from the reference: the constructor signature (index.py:59-77, ``dim=`` alias 80-84),
``train`` / ``partial_train`` / ``index`` / ``update`` / ``delete`` / ``search`` /
``search_by_vectors`` / ``search_numpy`` / ``encode`` / ``decode`` / ``clear`` / ``close`` /
``stat`` / ``is_trained`` / ``total_docs`` / ``index_size``, the error behaviour
(``RuntimeError('The indexer is not trained ...')``, index.py:284-285, 349-350; read-only index logs
and returns, 280-282), the result shape (``doc.matches = DocumentArray[Document(id=...)]`` with
``scores[metric.name.lower()].value = dist``, container.py:226-233) and the on-disk location of the
trained codec (``data_path/parameters-<md5>/pq_codec.params``, index.py:574-599, 679-687).

Changed on purpose: the vector index per cell is the exhaustive
GPU scan ``PQFlatGpuIndex`` instead of an HNSW graph walked one query at a time
(container.py:48-59, 214); ALL queries of a ``search`` call go through one batched launch.

Without ``n_subvectors`` (the reference's default: an un-quantised float ``HnswIndex``) the index is ``FlatGpuIndex``: exact
float32 search -- an f32 MFMA filter with a proven slack, then exact sums.  No codec, nothing to train.
With ``n_cells > 1`` and ``ivf_prune=True`` it is ``IvfFlatGpuIndex``: cells over the float vectors -- a ``VQCodec`` to train, and
a search that scans each query's ``n_probe`` nearest cells and answers those rows exactly.

With ``graph=True, build='gpu'`` it is ``HnswFlatGpuIndex``, a level-0 HNSW graph over the float vectors.  A
search with a ``filter`` is answered exactly by default; ``filter_search='graph'`` answers it on the graph as hnswlib's filtered search
does (the walk routes through every row, only rows that pass the filter are listed), except for filters that keep too few rows for the
walk to pay (``HnswFlatGpuIndex.FILTER_WALK_MIN_FRACTION``), which stay exact.  The graph over PQ codes (``n_subvectors=M, graph=True``:
``HnswPQGpuIndex``) takes the same option with a floor of its own (``HnswPQGpuIndex.FILTER_WALK_MIN_FRACTION``).

``n_cells > 1`` (index.py:125-133, 458-483): a ``VQCodec`` coarse quantiser assigns every vector to a cell and ONE
``IvfPQGpuIndex`` holds all cells.  Like the reference (``n_probe = max(n_probe, n_cells)``, index.py:94) a search
visits every cell, so results equal the single-cell index; ``ivf_prune=True`` (kwarg) makes the search honour
``n_probe`` -- the pruned scan of SURVEY.md section 8f's follow-on.

``n_components=K, projector='gpu'`` (index.py:111-123): a ``ProjectorCodec`` in front of every index above -- a
PCA fitted on the GPU (covariance accumulated exactly, eigen-decomposition on the host: the subspace sklearn's PCA finds, by another
route -- hence the explicit opt-in; ``n_components`` alone still raises).  ``index`` / ``update`` / ``search`` upload the rows once and project
them on the device; the index and the PQ codec have dimension K; stored documents keep their original embeddings.
Changed on purpose: ``train`` fits the projector first and trains the VQ / PQ codecs on the PROJECTED training rows (the reference hands
them the raw ``x``, index.py:212-228, which cannot train a PQ codec of dimension K); ``partial_train`` shows the other codecs each batch
through the projector's state after that batch -- a caller who wants them trained against one fixed projection trains the projector first.

Out of scope of this tier: RocksDB/SQLite
persistence of documents, remote backup.  Documents and tags live in memory; the Mongo-style ``filter`` dict is
evaluated on the host and handed to the GPU scan as a row bitmap (section 8f-3) -- unless it names declared ``columns`` only:
those are kept as typed device arrays beside the vectors (``ColumnStore``, columns.py), the filter compiles to a predicate program
and ONE kernel evaluates it into the bitmap the indexes read (``annlite_filter_eval``).  The rows selected
are the same; ``filter_eval='host'`` keeps the host path, ``last_filter_eval`` says which one answered.  ``filter()`` /
``get_docs()`` then select their page (``order_by``, ``offset``, ``limit``) on the device too (``ColumnStore.page``, DESIGN.md section
3.10.1); ``last_filter_page`` says whether they did.  ``filter=`` of the searches may also be a list with a filter PER QUERY: equal
filters form a group, each distinct one is evaluated once, and the float index answers the batch in one search under all of them
(``search_batch_grouped``, DESIGN.md section 3.6, "a filter per query"; ``last_filter_batch`` / ``last_filter_groups``).
"""
import hashlib
import logging
import sqlite3
import warnings
import weakref
from pathlib import Path
from typing import Dict, List, Optional, Union

import numpy as np
import torch

from . import ops
from .columns import ColumnStore, RowMask
from .core.codec.pq import PQCodec
from .core.index.pq_flat_gpu import PQFlatGpuIndex
from .core.index.row_store import group_filters
from .enums import Metric
from .filter import select as _filter_select

try:  # real docarray when present (it is not in this image)
    from docarray import Document, DocumentArray
    from docarray.math.ndarray import to_numpy_array

    if not isinstance(Document, type):  # (a test harness may have stubbed the module)
        raise ImportError('docarray is stubbed')
    LazyMatches = None  # (real docarray: ``Document.matches`` takes its own DocumentArray type -- matches are built eagerly)
except Exception:  # pragma: no cover - depends on the environment
    from .docarray_compat import Document, DocumentArray, LazyMatches, to_numpy_array

logger = logging.getLogger('annlite_amd')

MAX_TRAINING_DATA_SIZE = 10240  # index.py:23


class AnnLite:
    """MI355X-native drop-in for :class:`annlite.AnnLite`: the PQ search path, and exact search over float vectors.

    :param n_dim: dimensionality of input vectors (divisible by ``n_subvectors``)
    :param metric: 'euclidean', 'inner_product' or 'cosine'
    :param n_subvectors: number of PQ sub-quantisers = bytes per stored vector; ``None`` (the default, as in the reference)
        keeps the float vectors themselves and searches them exactly (``FlatGpuIndex``; ``n_cells > 1`` needs ``ivf_prune=True``:
        ``IvfFlatGpuIndex``) or, with ``graph=True, build='gpu'``, through a level-0 HNSW graph over them (``HnswFlatGpuIndex``)
    :param n_clusters: codewords per sub-quantiser (default 256)
    :param n_components: with ``projector='gpu'`` (kwarg): project the vectors to this many PCA components on the GPU in front of
        whichever index the other arguments select (``ProjectorCodec``; trained by ``train`` / ``partial_train``); ``n_components``
        without ``projector='gpu'`` raises ``NotImplementedError`` (the fit is not sklearn's: an explicit opt-in)
    :param rerank: keep the float vectors in HBM and re-score ADC candidates exactly (kwarg, rides
        the reference's ``**kwargs`` channel to the index, container.py:56).  With ``n_cells > 1`` and ``ivf_prune=True`` the same channel
        takes ``rerank_bound_rank`` / ``rerank_split`` (the candidate pool of the pruned search's re-rank: ``IvfPQGpuIndex``)
    :param filter_search: ``'exact'`` (default) or ``'graph'`` (kwarg, same channel; the two graph indexes -- ``graph=True`` with or
        without ``n_subvectors`` --, ignored by the other indexes): how a search that carries a ``filter`` is answered -- by the exact
        filtered search, or by the graph walk that lists only the rows the filter admits (``HnswFlatGpuIndex.search_batch``,
        ``HnswPQGpuIndex.search_batch``)
    :param flat_filter: ``'f32'`` (default) or ``'bf16x3'``, with ``centre`` (``'mean'``, ``None`` or an array) (kwargs, same channel;
        the float indexes -- no ``n_subvectors`` --, dropped for the indexes over PQ codes, ignored with ``n_cells > 1``): the filter
        of the exact float search; ``'bf16x3'`` is the one for data with a large common offset (``FlatGpuIndex``)
    :param filter_route: ``'mask'`` (default), ``'rows'`` or ``'auto'`` (kwarg, same channel; the float indexes, dropped for the indexes
        over PQ codes): whether a filtered exact search over float vectors scans the table under the filter's bitmap or only the rows
        the filter selects, compacted into a list first -- the same answer bit for bit (``FlatGpuIndex``; the float graph's exact
        fallback and the cells' every-cell search inherit it)
    :param cell_filter: ``'f32'`` (default) or ``'bf16x3'`` (kwarg, same channel; ``n_cells > 1`` with ``ivf_prune=True`` and no
        ``n_subvectors``, dropped for every other index): the filter over the cell tiles of ``IvfFlatGpuIndex``; ``'bf16x3'`` centres
        every tile on its cell's centroid -- the one for data with a common offset, the same answer bit for bit
    :param dtype: ``np.float32`` (default) or ``np.float16`` (kwarg, same channel; the reference's ``dtype`` of its index plug-ins):
        without ``n_subvectors``, ``n_cells > 1`` and ``graph`` it reaches ``FlatGpuIndex``, which then stores its rows in half
        precision -- half the HBM, the answer of the f32 index over the rounded rows bit for bit, its own filter ``'f16x2'`` (no
        ``flat_filter='bf16x3'``, no ``centre``: centre data with a common offset before adding it).  The float graph
        (``graph=True``) and the cells over floats (``n_cells > 1``) read f32 rows only and raise ``NotImplementedError`` for
        ``np.float16``; the indexes over PQ codes ignore ``dtype``, as before.  ``np.int8`` with ``int8_scale`` (a power of two, same
        channel; default 1.0, ``2**-7`` for cosine) rides the same way: ``FlatGpuIndex`` then stores int8 codes -- a quarter of the HBM,
        the answer of the f32 index over the rows ``int8_scale * code`` bit for bit, its own filter ``'i8x3'``; the float graph and
        the cells over floats raise ``NotImplementedError``, the indexes over PQ codes drop both keywords
    :param columns: ``[(name, type), ...]`` (or ``filterable_attrs={name: type}``): the tags a filter may name and have evaluated on
        the device -- ``int`` / ``bool``, ``float`` and ``str`` columns (``ColumnStore``); tags that are not declared stay filterable
        on the host, as before
    :param filter_eval: ``'auto'`` (default; kwarg): a filter that compiles over the declared columns is evaluated by
        ``annlite_filter_eval``, any other by ``filter.select``; ``'host'``: ``filter.select`` always.  ``last_filter_eval`` reports
        ``'gpu'`` / ``'host'`` for the last filter (``None`` before the first).  With ``'auto'`` ``filter()`` / ``get_docs()`` also select
        their page -- ``order_by`` a declared column or none, ``offset``, ``1 <= limit <= 4096`` -- on the device
        (``annlite_order_page`` / ``annlite_bitmap_page``); ``last_filter_page`` reports ``'gpu'`` / ``'host'`` for the last page
    """

    def __init__(
        self,
        n_dim: int,
        metric: Union[str, Metric] = 'cosine',
        n_cells: int = 1,
        n_subvectors: Optional[int] = None,
        n_clusters: Optional[int] = 256,
        n_probe: int = 16,
        n_components: Optional[int] = None,
        initial_size: Optional[int] = None,
        expand_step_size: int = 10240,
        columns: Optional[Union[Dict, List]] = None,
        filterable_attrs: Optional[Dict] = None,
        data_path: Union[Path, str] = Path('./data'),
        create_if_missing: bool = True,
        read_only: bool = False,
        verbose: bool = False,
        **kwargs,
    ):
        logger.setLevel(logging.DEBUG if verbose else logging.INFO)
        if 'dim' in kwargs:
            warnings.warn('The argument `dim` will be deprecated, please use `n_dim` instead.')
            n_dim = kwargs.pop('dim')
        projector = kwargs.pop('projector', None)
        if projector is not None and projector != 'gpu':
            raise NotImplementedError(f"projector={projector!r}: the PCA projector exists on the GPU only, pass projector='gpu'")
        use_projector = bool(n_components) and projector == 'gpu'
        if n_subvectors and use_projector:  # index.py:143-146: the PQ codec sees the projected vectors
            assert n_components % n_subvectors == 0, '"n_components" needs to be divisible by "n_subvectors"'
        elif n_subvectors:
            assert n_dim % n_subvectors == 0, '"n_dim" needs to be divisible by "n_subvectors"'
        assert n_cells >= 1
        if n_components and not use_projector:
            # the reference fits sklearn's PCA / IncrementalPCA; the projector here is an eigen-decomposition of an exactly accumulated
            # covariance (the same subspace by another route) and is therefore opted into by name
            raise NotImplementedError("n_components (PCA projector) is served by the GPU projector only: pass projector='gpu' "
                                      "(a fit by covariance eigen-decomposition, not sklearn's SVD / IncrementalPCA)")
        assert not (projector and not n_components), "projector='gpu' needs n_components"
        if not n_subvectors:
            # the reference's default configuration: an un-quantised float index (FlatGpuIndex: exact search)
            if n_cells > 1 and not kwargs.get('ivf_prune'):
                # (every cell visited -- all the reference does with its cells -- is the exact index with n_cells=1)
                raise NotImplementedError('n_cells > 1 without n_subvectors (cells over float vectors) is the pruned exact search: pass '
                                          'ivf_prune=True (a query then scans its n_probe nearest cells), or n_cells=1 for the exhaustive '
                                          'exact float32 index, or n_subvectors')
            if kwargs.get('graph'):
                # the float HNSW graph (HnswFlatGpuIndex): only the GPU-built level-0 graph exists over floats
                # -- there is no host library for it -- so it is opted into with the PQ graph's `build` vocabulary
                if n_cells > 1:
                    raise NotImplementedError('graph=True and n_cells > 1 cannot be combined (the float graph is one index over all rows)')
                if kwargs.get('build') != 'gpu':
                    raise NotImplementedError("graph=True without n_subvectors (a float HNSW graph) exists as the GPU-built level-0 graph "
                                              "only: pass build='gpu' (build='host' needs n_subvectors: the graph over PQ codes)")
        self.n_dim = n_dim
        self.n_components = n_components
        self.n_subvectors = n_subvectors
        self.n_clusters = n_clusters
        self.n_probe = max(n_probe, n_cells)  # index.py:94: the reference visits every cell
        self._n_probe_arg = n_probe
        self._ivf_prune = bool(kwargs.pop('ivf_prune', False))
        # devices=[0, 1, ...]: the code table row-sharded over these GPUs behind this ONE object (MultiGpuPQIndex: one
        # process, one stream per device, packed per-shard top-k merged on the first device); default: the current device
        self._devices = kwargs.pop('devices', None)
        self._shard_block = int(kwargs.pop('shard_block', 65536))
        self.n_cells = n_cells
        if isinstance(metric, str):
            metric = Metric.from_string(metric)
        self.metric = metric
        self.read_only = read_only

        data_path = Path(data_path)
        if create_if_missing:
            data_path.mkdir(parents=True, exist_ok=True)
        self.data_path = data_path

        self._projector_codec = None
        if use_projector:  # index.py:111-123
            from .core.codec.projector import ProjectorCodec

            if self._projector_codec_path.exists():
                logger.info(f'Load pre-trained projector codec (n_components={self.n_components}) from {self.model_path}')
                self._projector_codec = ProjectorCodec.load(self._projector_codec_path)
            else:
                self._projector_codec = ProjectorCodec(n_dim, n_components=n_components)
        self._index_dim = n_components if use_projector else n_dim  # what the indexes and the PQ codec see

        self._pq_codec = None
        if not n_subvectors:
            pass  # (no codec: nothing to train)
        elif self._pq_codec_path.exists():
            logger.info(f'Load trained PQ codec (n_subvectors={self.n_subvectors}) from {self.model_path}')
            self._pq_codec = PQCodec.load(self._pq_codec_path)
        else:
            self._pq_codec = PQCodec(dim=self._index_dim, n_subvectors=n_subvectors, n_clusters=n_clusters, metric=metric)

        self._vq_codec = None
        if n_cells > 1:  # index.py:125-133
            from .core.codec.vq import VQCodec

            if self._vq_codec_path.exists():
                logger.info(f'Load trained VQ codec (K={self.n_cells}) from {self.model_path}')
                self._vq_codec = VQCodec.load(self._vq_codec_path)
            else:
                self._vq_codec = VQCodec(self.n_cells, metric=self.metric)

        if columns is not None:
            filterable_attrs = {n: t for n, t in (columns.items() if isinstance(columns, dict) else columns)}
        self.filterable_attrs = filterable_attrs or {}
        # the declared columns as device arrays of the row range (columns.py; nothing is allocated before the first rows arrive).
        # filter_eval='auto': a filter that compiles over them is evaluated on the device; 'host': `filter.select`, always
        self.filter_eval = kwargs.pop('filter_eval', 'auto')
        if self.filter_eval not in ('auto', 'host'):
            raise ValueError(f"filter_eval={self.filter_eval!r}: 'auto' (the device where the filter compiles) or 'host'")
        self._columns = ColumnStore(self.filterable_attrs)
        self.last_filter_eval = None  # 'gpu' / 'host': what evaluated the last filter (None: no filter yet)
        self.last_filter_page = None  # 'gpu' / 'host': what selected the last page of filter() / get_docs() (None: no call yet)
        self.last_filter_batch = None   # 'grouped' / 'looped': how the last search with a filter PER QUERY was answered (None: one filter)
        self.last_filter_groups = None  # the distinct filters of that search (None: `filter` was not a list)

        self._index_kwargs = dict(initial_size=initial_size, expand_step_size=expand_step_size, **kwargs)
        self._vec_indexes = [self._new_index()]
        # in-memory stand-ins for CellTable / DocStorage (offset <-> doc id, tags, documents)
        self._offset2id: List[Optional[str]] = []
        self._id2offset: Dict[str, int] = {}
        self._tags: List[Optional[dict]] = []
        self._docs: Dict[str, object] = {}
        self._tomb: Dict[int, tuple] = {}  # offset -> (doc id, document) of deleted rows: what pending lazy match lists still name
        self._live_resolvers = weakref.WeakSet()  # resolvers of match lists not yet read: tombstones are kept only while one is alive
        if self.is_trained and self.snapshot_path is not None:  # index.py:194-195: restore what `dump()` left
            self._rebuild_index_from_local()

    def _new_index(self) -> PQFlatGpuIndex:
        """The per-cell vector index (container.py:48-59 builds ``HnswIndex(...)`` there).  Default: the exhaustive
        GPU scan; ``AnnLite(..., graph=True, ef_search=..., max_connection=..., ef_construction=...)`` selects the
        HNSW-over-PQ index with the reference's knobs (graph walked on the GPU, BASELINE config 5)."""
        kw = dict(self._index_kwargs)
        if self._pq_codec is None:
            from .core.index.flat_gpu import FlatGpuIndex

            if self._devices is not None and len(self._devices) > 1:
                warnings.warn('devices= is ignored for the float index (it lives on the current device)')
            graph = kw.pop('graph', False)
            for name in ('rerank', 'rerank_pool', 'skewed'):  # (PQ index options: the float index is exact already)
                kw.pop(name, None)
            if graph:  # (build='gpu', n_cells == 1: the constructor refuses the rest)
                from .core.index.hnsw_flat_gpu import HnswFlatGpuIndex

                kw.pop('cell_filter', None)  # (the cells' option)

                return HnswFlatGpuIndex(dim=self._index_dim, metric=self.metric, **kw)
            kw.pop('build', None)
            kw.pop('filter_search', None)  # (the float graph's option: these indexes answer a filter exactly)
            if self._vq_codec is not None:  # (ivf_prune=True: the constructor refuses cells over floats without it)
                from .core.index.ivf_flat_gpu import IvfFlatGpuIndex

                return IvfFlatGpuIndex(dim=self._index_dim, metric=self.metric, vq_codec=self._vq_codec, n_probe=self._n_probe_arg, **kw)
            kw.pop('cell_filter', None)  # (the cells' option)
            return FlatGpuIndex(dim=self._index_dim, metric=self.metric, **kw)
        if not (self._vq_codec is None and kw.get('graph')):
            kw.pop('filter_search', None)  # (the graph indexes' option: the other indexes over PQ codes answer a filter exactly)
        for name in ('flat_filter', 'centre', 'cell_filter', 'int8_scale', 'filter_route'):  # (the float indexes' options: nothing over PQ codes runs that filter)
            kw.pop(name, None)
        if self._devices is not None and len(self._devices) > 1 and (self._vq_codec is not None or kw.get('graph')):
            warnings.warn('devices= is ignored for n_cells > 1 and graph=True indexes (they live on the current device)')
        if self._vq_codec is not None:
            from .core.index.ivf_pq_gpu import IvfPQGpuIndex

            assert not kw.pop('graph', False), 'graph=True and n_cells > 1 cannot be combined'
            return IvfPQGpuIndex(dim=self._index_dim, metric=self.metric, pq_codec=self._pq_codec, vq_codec=self._vq_codec,
                                 n_probe=self._n_probe_arg if self._ivf_prune else None, **kw)
        if kw.pop('graph', False):
            from .core.index.hnsw_pq_gpu import HnswPQGpuIndex

            return HnswPQGpuIndex(dim=self._index_dim, metric=self.metric, pq_codec=self._pq_codec, **kw)
        if self._devices is not None and len(self._devices) > 1:
            from .core.index.multi_gpu import MultiGpuPQIndex

            return MultiGpuPQIndex(dim=self._index_dim, metric=self.metric, pq_codec=self._pq_codec, devices=self._devices,
                                   block=self._shard_block, **kw)
        return PQFlatGpuIndex(dim=self._index_dim, metric=self.metric, pq_codec=self._pq_codec, **kw)

    # ------------------------------------------------------------------ bookkeeping (index.py:574-599, 952-963)
    @property
    def params_hash(self):
        model_metas = (f'n_dim: {self.n_dim} metric: {self.metric} n_cells: {self.n_cells} '
                       f'n_components: {self.n_components} n_subvectors: {self.n_subvectors}')
        return hashlib.md5(f'{model_metas}'.encode()).hexdigest()

    @property
    def model_path(self):
        return self.data_path / f'parameters-{self.params_hash}'

    @property
    def _pq_codec_path(self):
        return self.model_path / 'pq_codec.params'

    @property
    def _vq_codec_path(self):
        return self.model_path / 'vq_codec.params'  # index.py:589-591

    @property
    def _projector_codec_path(self):
        return self.model_path / 'projector_codec.params'  # index.py:597-599

    @property
    def is_trained(self) -> bool:
        if self._projector_codec is not None and not self._projector_codec.is_trained:  # index.py:927
            return False
        if self._vq_codec is not None and not self._vq_codec.is_trained:  # index.py:929-930
            return False
        if not self.n_subvectors:  # the float index has nothing to train (index.py:925-932: no codec -> trained)
            return True
        return bool(self._pq_codec is not None and self._pq_codec.is_trained)

    @property
    def total_docs(self) -> int:
        return len(self._id2offset)

    @property
    def index_size(self) -> int:
        return sum(idx.size for idx in self._vec_indexes)

    @property
    def stat(self):
        return {
            'total_docs': self.total_docs, 'index_size': self.index_size, 'n_cells': self.n_cells,
            'n_dim': self.n_dim, 'n_components': self.n_components, 'metric': self.metric.name,
            'is_trained': self.is_trained,
        }

    def vec_index(self, cell_id: int = 0) -> PQFlatGpuIndex:
        return self._vec_indexes[cell_id]

    def _project(self, x):
        """container.py:210, 245, 271: what the vector index is given.  With a projector the rows go up once and are projected there
        (``annlite_affine_rows``); the index receives the device tensor.  Stored documents keep their original embeddings."""
        if self._projector_codec is None:
            return x
        return self._projector_codec.encode(ops.to_dev(x, torch.float32))

    def _sanity_check(self, x):
        assert x.ndim == 2, 'inputs must be a 2D array'
        assert x.shape[1] == self.n_dim, (
            f'inputs must have the same dimension as the index , got {x.shape[1]}, expected {self.n_dim}')
        return x.shape

    # ------------------------------------------------------------------ training (index.py:197-272, 679-687)
    def train(self, x, auto_save: bool = True, force_train: bool = False):
        self._sanity_check(x)
        if self.is_trained and not force_train:
            logger.warning('The indexer has been trained or is not trainable. Please use ``force_train=True`` to retrain.')
            return
        x = x if isinstance(x, torch.Tensor) else np.ascontiguousarray(x, dtype=np.float32)
        if self._projector_codec is not None:  # index.py:212-216
            logger.info(f'Start training Projector codec (n_components={self.n_components}) with {x.shape[0]} data...')
            x = ops.to_dev(x, torch.float32)
            self._projector_codec.fit(x)
            x = self._projector_codec.encode(x)  # (changed on purpose: the other codecs are trained on what they will be given)
        if self._vq_codec is not None:  # index.py:218-222
            logger.info(f'Start training VQ codec (K={self.n_cells}) with {x.shape[0]} data...')
            self._vq_codec.fit(x)
        if self._pq_codec is not None:  # (the float index has no PQ codec: with cells only the VQ codec is trained)
            self._pq_codec.fit(x)
        if auto_save and (self._pq_codec is not None or self._vq_codec is not None or self._projector_codec is not None):
            self.dump_model()

    def partial_train(self, x, auto_save: bool = True, force_train: bool = False):
        self._sanity_check(x)
        if self.is_trained and not force_train:
            logger.warning('The annlite has been trained or is not trainable. Please use ``force_train=True`` to retrain.')
            return
        if self._projector_codec is not None:  # index.py:253-257
            # the other codecs see this batch through the projector's state after it: a caller who wants them trained against ONE
            # projection trains the projector first (all batches, or `train`), then the rest
            x = ops.to_dev(x, torch.float32)
            self._projector_codec.partial_fit(x)
            x = self._projector_codec.encode(x)
        if self._vq_codec is not None:  # index.py:259-263
            self._vq_codec.partial_fit(x)
            self._vq_codec.build_codebook()
        if self._pq_codec is not None:
            self._pq_codec.partial_fit(x)
            self._pq_codec.build_codebook()
        if auto_save and (self._pq_codec is not None or self._vq_codec is not None or self._projector_codec is not None):
            self.dump_model()

    def dump_model(self):
        self.model_path.mkdir(parents=True, exist_ok=True)
        if self._projector_codec is not None:
            self._projector_codec.dump(self._projector_codec_path)  # index.py:682-683
        if self._pq_codec is not None:
            self._pq_codec.dump(self._pq_codec_path)
        if self._vq_codec is not None:
            self._vq_codec.dump(self._vq_codec_path)  # index.py:684-685

    # ------------------------------------------------------------------ snapshots (index.py:600-637, 689-714, 769-777)
    @property
    def index_path(self) -> Path:
        import datetime

        stamp = datetime.datetime.utcnow().isoformat('#', 'seconds')
        return self.data_path / f'snapshot-{self.params_hash}' / f'{stamp}-SNAPSHOT'

    @property
    def snapshot_path(self) -> Optional[Path]:
        paths = sorted((self.data_path / f'snapshot-{self.params_hash}').glob('*-SNAPSHOT'), key=lambda x: x.name)
        return paths[-1] if paths else None

    def dump_index(self):
        """index.py:689-710: ``cell_0.hnsw`` = the vector index (own format: codes, validity, cells / graph / float
        vectors where present), ``cell_0.db`` = the offset <-> document table (in-memory store, pickled)."""
        import pickle
        import shutil

        path = self.index_path
        logger.info(f'Save the indexer to {path}')
        try:
            if path.exists():
                shutil.rmtree(path)
            path.mkdir(parents=True)
            self.vec_index(0).dump(path / 'cell_0.hnsw')
            with open(path / 'cell_0.db', 'wb') as f:
                pickle.dump({'offset2id': self._offset2id, 'tags': self._tags, 'docs': self._docs}, f, protocol=4)
        except Exception as ex:
            logger.error(f'Failed to dump the indexer, {ex!r}')
            if path.exists():
                shutil.rmtree(path)
            raise

    def dump(self):
        self.dump_model()
        self.dump_index()

    def _rebuild_index_from_local(self):
        import pickle

        snap = self.snapshot_path
        logger.info(f'Load the indexer from snapshot {snap}')
        try:
            self.vec_index(0).load(snap / 'cell_0.hnsw')
        except (AssertionError, KeyError, FileNotFoundError) as ex:
            # the vector index file carries its own 'format' (flat / cells / graph / multi-GPU header + .shard<g> files): a
            # snapshot is reopened with the layout arguments of the AnnLite that wrote it
            raise RuntimeError(
                f'snapshot {snap} does not fit this index ({type(self.vec_index(0)).__name__}): reopen it with the same '
                f'devices= / shard_block= / n_cells / graph arguments it was dumped with ({ex!r})') from ex
        with open(snap / 'cell_0.db', 'rb') as f:
            st = pickle.load(f)
        self._offset2id, self._tags, self._docs, self._tomb = st['offset2id'], st['tags'], st['docs'], {}
        self._columns.clear()  # (the columns are not part of the snapshot: refilled from the restored tags)
        self._columns.append(self._tags)
        self._offset2int = None
        self._id2offset = {d: o for o, d in enumerate(self._offset2id) if d is not None}

    def backup(self, target_name: Optional[str] = None, token: Optional[str] = None):
        """index.py:652-664: local backup = ``dump()``; the remote (hub) target is outside this tier."""
        if target_name:
            raise NotImplementedError('remote backup (Jina hub artifacts) is out of scope (SURVEY.md section 2 row 22)')
        logger.info('dump to local ...')
        self.dump()

    def restore(self, source_name: Optional[str] = None, token: Optional[str] = None):
        """index.py:666-677"""
        if source_name:
            raise NotImplementedError('remote restore (Jina hub artifacts) is out of scope (SURVEY.md section 2 row 22)')
        if self.snapshot_path is not None:
            logger.info('restore Annlite from local')
            self._rebuild_index_from_local()

    # ------------------------------------------------------------------ index / update / delete
    def index(self, docs, **kwargs):
        """index.py:274-295 -> CellContainer.insert (container.py:262-308): offsets are dense row ids."""
        if self.read_only:
            logger.error('The indexer is readonly, cannot add new documents')
            return
        if not self.is_trained:
            raise RuntimeError('The indexer is not trained, cannot add new documents')
        x = to_numpy_array(docs.embeddings)
        self._sanity_check(x)
        # the reference's cell table declares `_doc_id TEXT NOT NULL UNIQUE` (storage/table.py:203): a document id
        # that is already indexed -- or twice in this batch -- is an IntegrityError there; nothing is inserted
        seen = set()
        for d in docs:
            if d.id in self._id2offset or d.id in seen:
                raise sqlite3.IntegrityError(f'UNIQUE constraint failed: _doc_id (id={d.id})')
            seen.add(d.id)
        first = len(self._offset2id)
        offsets = np.arange(first, first + len(docs), dtype=np.int64)
        # vectors first: if the device call fails no offset exists without codes
        self.vec_index(0).add_with_ids(self._project(np.ascontiguousarray(x, dtype=np.float32)), offsets)
        self._offset2int = None
        for d in docs:
            self._id2offset[d.id] = len(self._offset2id)
            self._offset2id.append(d.id)
            self._tags.append(dict(d.tags) if getattr(d, 'tags', None) else {})
            self._docs[d.id] = d
        if self._columns.kinds:
            self._columns.append(self._tags[first:])

    def update(self, docs, raise_errors_on_not_found: bool = False, insert_if_not_found: bool = True, **kwargs):
        """index.py:297-332: delete + re-insert under a fresh offset (container.py:323-375)."""
        if self.read_only:
            logger.error('The indexer is readonly, cannot update documents')
            return
        if not self.is_trained:
            raise RuntimeError('The indexer is not trained, cannot add new documents')
        new_docs = DocumentArray()
        for d in docs:
            if d.id in self._id2offset:
                self.delete([d.id])
                new_docs.append(d)
            elif raise_errors_on_not_found and not insert_if_not_found:  # container.py:349-365
                raise Exception(f'The document (id={d.id}) cannot be updated as it is not found in the index')
            elif not (raise_errors_on_not_found or insert_if_not_found):
                warnings.warn(f'The document (id={d.id}) cannot be updated as it is not found in the index', RuntimeWarning)
            elif insert_if_not_found:
                new_docs.append(d)
        if len(new_docs):
            self.index(new_docs)

    def delete(self, docs, raise_errors_on_not_found: bool = False):
        # ids or documents (the reference takes either, index.py:389-414; a DocumentArray may itself be a list subclass)
        ids = [d if isinstance(d, str) else d.id for d in docs]
        offs = []
        # tombstones exist for match lists handed out and not read yet; once none is left (read, or dropped by the caller) nothing
        # can ask for a deleted row again -- a later search never returns it -- and the map is emptied instead of growing for ever
        pending = len(self._live_resolvers) > 0
        if not pending and self._tomb:
            self._tomb.clear()
        for doc_id in ids:
            off = self._id2offset.pop(doc_id, None)
            if off is None:
                if raise_errors_on_not_found:
                    raise Exception(f'The document (id={doc_id}) cannot be updated as it is not found in the index')
                continue
            self._offset2id[off] = None
            self._offset2int = None
            self._tags[off] = None
            doc = self._docs.pop(doc_id, None)
            if pending:
                self._tomb[off] = (doc_id, doc)
            offs.append(off)
        if offs:
            self.vec_index(0).delete(offs)
            self._columns.drop(offs)

    def clear(self):
        self.vec_index(0).reset()
        self._offset2id, self._id2offset, self._tags, self._docs, self._tomb = [], {}, [], {}, {}
        self._offset2int = None
        self._columns.clear()

    def close(self):
        pass

    # ------------------------------------------------------------------ search
    def _filter_offsets(self, filter: Optional[dict]):
        """The rows a filter selects: a ``RowMask`` where the filter compiles over the declared columns (evaluated on the device), else
        the offsets ``filter.select`` finds (None: no filter).  The same rows either way."""
        if not filter:
            return None
        if self.filter_eval == 'auto' and len(self._columns) > 0:
            program = self._columns.compile(filter)
            if program is not None:
                self.last_filter_eval = 'gpu'
                return self._columns.evaluate(program)
        self.last_filter_eval = 'host'
        return np.asarray(_filter_select(self._tags, filter), dtype=np.int64)

    def _search_arrays_grouped(self, query_np, filters, group_of, limit):
        """``_search_arrays`` with a filter per query: ``filters`` are the distinct ones (``group_filters``), each evaluated ONCE -- on
        the device where it compiles, on the host where it does not --, and the vector index answers the batch under all of them
        (``search_batch_grouped``; DESIGN.md section 3.6, "a filter per query").  ``[B, k]`` arrays, ``k = min(limit, index_size)``:
        a query whose filter selects fewer rows has the (+inf, -1) tail the callers cut."""
        B = query_np.shape[0]
        selections, any_host = [], False
        for flt in filters:
            selections.append(self._filter_offsets(flt))
            any_host = any_host or (flt is not None and self.last_filter_eval == 'host')
        if any_host:
            self.last_filter_eval = 'host'
        k = min(int(limit), max(self.index_size, 0))
        if k <= 0:
            return np.full((B, 0), np.inf, np.float32), np.full((B, 0), -1, np.int64)
        index = self.vec_index(0)
        if not hasattr(index, 'search_batch_grouped'):
            raise NotImplementedError(f'a filter per query is not implemented over {type(index).__name__} (devices=)')
        d, i = index.search_batch_grouped(self._project(np.ascontiguousarray(query_np, dtype=np.float32)), limit=k, selections=selections,
                                          group_of=group_of)
        self.last_filter_batch = index.last_filter_batch
        if isinstance(d, torch.Tensor):
            d, i = d.cpu().numpy(), i.cpu().numpy()
        return d, i

    def _search_arrays(self, query_np, filter, limit):
        self._sanity_check(query_np)
        self.last_filter_batch = self.last_filter_groups = None
        if isinstance(filter, (list, tuple)):  # a filter per query; all equal: the one-filter call below, as if it had been passed once
            filters, group_of = group_filters(filter, query_np.shape[0])
            self.last_filter_groups = len(filters)
            if len(filters) > 1:
                return self._search_arrays_grouped(query_np, filters, group_of, limit)
            filter = filters[0] if filters else None
        indices = self._filter_offsets(filter)
        if indices is not None and len(indices) == 0:
            B = query_np.shape[0]
            return np.full((B, 0), np.inf, np.float32), np.full((B, 0), -1, np.int64)
        n_avail = self.index_size if indices is None else len(indices)
        k = min(int(limit), max(n_avail, 0))  # container.py:118-120  limit=min(limit, cell_size)
        if k <= 0:
            B = query_np.shape[0]
            return np.full((B, 0), np.inf, np.float32), np.full((B, 0), -1, np.int64)
        d, i = self.vec_index(0).search_batch(self._project(np.ascontiguousarray(query_np, dtype=np.float32)), limit=k, indices=indices)
        if isinstance(d, torch.Tensor):  # (projected queries are device tensors, and so is their answer)
            d, i = d.cpu().numpy(), i.cpu().numpy()
        return d, i

    def search(self, docs, filter: Union[dict, list, tuple, None] = None, limit: int = 10, include_metadata: bool = True, **kwargs):
        """index.py:334-359: attaches ``doc.matches`` in place; one batched GPU launch for all docs.  ``filter``: one dict for the
        batch, or a list / tuple with a filter (a dict, ``{}`` or None) PER DOCUMENT (``search_by_vectors``)."""
        if not self.is_trained:
            raise RuntimeError('The indexer is not trained, cannot add new documents')
        query_np = to_numpy_array(docs.embeddings)
        match_dists, match_docs = self.search_by_vectors(query_np, filter=filter, limit=limit, include_metadata=include_metadata)
        for doc, matches in zip(docs, match_docs):
            doc.matches = matches

    def _resolver(self, include_metadata: bool):
        """(offsets, dists) of one query -> its match documents: container.py:226-233 (``Document(id=doc_id)``, the stored
        document's fields with ``include_metadata``, ``scores[metric].value = dist``)."""
        name = self.metric.name.lower()
        # (what a LAZY list resolves against later: offsets are never reused and `clear()` / a reload rebind these containers, so
        # the only mutation that can reach a pending list is `delete()` -- which leaves the row's id and document in `_tomb`)
        offset2id, docs, tomb = self._offset2id, self._docs, self._tomb
        # the in-repo stand-in's factory (the score object is made when first read).  Gated on the stand-in itself: the real
        # docarray < 0.30 also has a ``Document.match`` -- its nearest-neighbour matcher, a different function altogether
        fast = Document.match if LazyMatches is not None else None

        def resolve(offs, dists):
            out = []
            for dist, off in zip(dists, offs.tolist() if hasattr(offs, 'tolist') else offs):
                doc_id = offset2id[off]
                if doc_id is None:  # deleted since the search: the match still is what it was when the search ran
                    doc_id, src = tomb.get(off, (None, None))
                    src = src if include_metadata else None
                else:
                    src = docs.get(doc_id) if include_metadata else None
                if fast is not None:
                    doc = fast(doc_id, name, dist) if src is None else fast(doc_id, name, dist, getattr(src, 'embedding', None),
                                                                            getattr(src, 'tags', None))
                else:
                    doc = Document(id=doc_id) if src is None else Document(id=doc_id, embedding=getattr(src, 'embedding', None),
                                                                           tags=dict(getattr(src, 'tags', {}) or {}))
                    doc.scores[name].value = dist
                out.append(doc)
            return out

        self._live_resolvers.add(resolve)
        return resolve

    @staticmethod
    def _valid_rows(d: np.ndarray, i: np.ndarray):
        """Per query the valid prefix of its result row (missing entries -- (+inf, -1) -- sort last): row views, no copies."""
        if d.shape[1] == 0 or bool((i[:, -1] >= 0).all()):
            return list(d), list(i)
        cnt = (i >= 0).sum(axis=1)
        return [d[b, :c] for b, c in enumerate(cnt)], [i[b, :c] for b, c in enumerate(cnt)]

    def search_by_vectors(self, query_np, filter: Union[dict, list, tuple, None] = None, limit: int = 10, include_metadata: bool = True):
        """index.py:361-387 -> CellContainer.search_cells (container.py:201-235).  ``filter`` may be a list or tuple of B entries, a
        filter (a dict, ``{}`` or None) PER QUERY -- any other length is a ``ValueError``: query b is answered as the call for that
        query alone with ``filter[b]`` is, the batch in one search where the index has one (``last_filter_batch``: ``'grouped'`` /
        ``'looped'``; ``last_filter_groups``: the distinct filters, each evaluated once).  The per-query match lists are LAZY
        (``LazyMatches``: the documents are built when a list is first read -- same ids, scores and metadata as the
        reference's eager loop, which costs tens of milliseconds per 1024-query batch next to a 1.4 ms scan)."""
        d, i = self._search_arrays(query_np, filter, limit)
        resolve = self._resolver(include_metadata)
        topk_dists, rows = self._valid_rows(d, i)
        if LazyMatches is not None:
            topk_docs = [LazyMatches(offs, dists, resolve) for offs, dists in zip(rows, topk_dists)]
        else:
            topk_docs = [DocumentArray(resolve(offs, dists)) for offs, dists in zip(rows, topk_dists)]
        return topk_dists, topk_docs

    def _offsets_as_int_ids(self) -> Optional[np.ndarray]:
        """offset -> ``int(doc_id)`` as one array (container.py:260 converts every returned id with ``int``): built once per
        state of the table, so that a batch's ids are ONE gather instead of B*k python conversions.  ``None`` when some
        stored id is not an integer literal (the conversion then happens per returned id, and raises like the reference's)."""
        cache = getattr(self, '_offset2int', None)
        if cache is None or len(cache) != len(self._offset2id):
            try:
                cache = np.fromiter((int(x) if x is not None else -1 for x in self._offset2id), dtype=np.int64,
                                    count=len(self._offset2id))
            except ValueError:
                return None
            self._offset2int = cache
        return cache

    def search_numpy(self, query_np, filter: Union[Dict, list, tuple, None] = {}, limit: int = 10, **kwargs):
        """index.py:485-522: (list of dists[k], list of doc-id arrays).  Ids are returned as the
        stored document ids converted with ``int`` like container.py:260.  ``filter``: one dict, or a filter per query
        (``search_by_vectors``)."""
        if not self.is_trained:
            raise RuntimeError('The indexer is not trained, cannot add new documents')
        d, i = self._search_arrays(query_np, filter, limit)
        valid = i >= 0
        table = self._offsets_as_int_ids()
        if table is None:  # (ids that are not integer literals: the reference's per-id conversion, and its ValueError)
            dists, rows = self._valid_rows(d, i)
            return dists, [np.array([int(self._offset2id[int(o)]) for o in r], dtype=int) for r in rows]
        ids_all = table[np.where(valid, i, 0)].astype(int, copy=False)
        if i.shape[1] == 0 or bool(valid.all()):
            return list(d), list(ids_all)
        cnt = valid.sum(axis=1)  # (missing entries sort last)
        return [d[b, :c] for b, c in enumerate(cnt)], [ids_all[b, :c] for b, c in enumerate(cnt)]

    def get_doc_by_id(self, doc_id: str):
        return self._docs.get(doc_id)

    def filter(self, filter: Optional[dict], limit: int = 10, offset: int = 0, order_by: Optional[str] = None,
               ascending: bool = True, include_metadata: bool = True):
        """index.py:389-423 -> CellContainer.filter_cells (container.py:146-199): the documents whose tags satisfy
        the filter, in insertion order or ordered by a tag, ``offset`` skipped, at most ``limit`` (<= 0: all).

        Where the rows are a device mask (or every row) and the page is one the device selects -- ``order_by`` a declared regular
        column or none, ``1 <= limit <= 4096`` --, only the page's offsets come to the host (``ColumnStore.page``: a radix select
        over the column); any other call is answered below, as before.  The same documents in the same
        order either way; ``last_filter_page`` says which one answered."""
        sel = self._filter_offsets(filter)
        page = None
        if self.filter_eval == 'auto' and (sel is None or isinstance(sel, RowMask)):
            page = self._columns.page(sel, order_by or None, ascending, offset, limit)
        self.last_filter_page = 'host' if page is None else 'gpu'
        if page is not None:
            return self._documents(page.tolist(), include_metadata)
        if sel is None:  # (no filter: every live row)
            offs = _filter_select(self._tags, {})
        else:
            offs = (sel.offsets() if isinstance(sel, RowMask) else sel).tolist()  # (ascending either way)
        if order_by:
            # documents without the tag sort as NULLs do in the reference's SQL ORDER BY (SQLite: NULLs first ascending,
            # last descending) instead of raising on a None comparison
            have = [o for o in offs if self._tags[o].get(order_by) is not None]
            miss = [o for o in offs if self._tags[o].get(order_by) is None]
            have = sorted(have, key=lambda o: self._tags[o].get(order_by), reverse=not ascending)
            offs = miss + have if ascending else have + miss
        offs = offs[offset:]
        if limit > 0:
            offs = offs[:limit]
        return self._documents(offs, include_metadata)

    def _documents(self, offs, include_metadata: bool):
        out = DocumentArray()
        for o in offs:
            doc_id = self._offset2id[o]
            out.append(self._docs[doc_id] if include_metadata else Document(id=doc_id))
        return out

    def get_docs(self, filter: Optional[dict] = None, limit: int = 10, offset: int = 0, order_by: Optional[str] = None,
                 ascending: bool = True):
        """index.py:433-456"""
        return self.filter(filter=filter, limit=limit, offset=offset, order_by=order_by, ascending=ascending,
                           include_metadata=True)

    # ------------------------------------------------------------------ codec passthrough (index.py:552-572)
    def encode(self, x):
        self._sanity_check(x)
        if self._pq_codec is None:
            raise RuntimeError('this index holds un-quantised float vectors: there is no PQ codec to encode with')
        if self._projector_codec is not None:  # index.py:554
            x = self._projector_codec.encode(x)
        return self._pq_codec.encode(x)

    def decode(self, x):
        assert len(x.shape) == 2
        if self._pq_codec is None:
            raise RuntimeError('this index holds un-quantised float vectors: there is no PQ codec to decode with')
        assert x.shape[1] == self.n_subvectors
        x = self._pq_codec.decode(x)
        if self._projector_codec is not None:  # index.py:569
            x = self._projector_codec.decode(x)
        return x
