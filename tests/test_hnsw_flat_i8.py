"""``HnswFlatGpuIndex(graph_rows='i8')``: the float graph over int8 rows is, bit for bit, the f32 graph index over the rows
``int8_scale * code`` -- same links, same ids, same distance bits, with and without a filter answered on the graph -- at a quarter of
the row bytes.  N = 12000 lies above ``BRUTE`` (8192): batches fed by the int8 walk are built.

COSINE: an f32 index normalises what it is fed, so feeding it decoded rows does not leave it the int8 index's rows (those are
normalised first, then quantised).  There the f32 twin's rows are overwritten with the int8 index's, decoded, and BOTH graphs are
linked again from nothing (``_rebuild_graph``), as tests/test_hnsw_flat_f16.py does."""
import numpy as np
import pytest

from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

N, D, B, K, EF = 12000, 32, 48, 10, 64
KNOBS = dict(ef_search=EF, max_connection=8, ef_construction=64, initial_size=4096)


def _same(got, want):
    (gd, gi), (wd, wi) = got, want
    return np.array_equal(gi, wi) and np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


@pytest.mark.parametrize('metric', ['EUCLIDEAN', 'COSINE'])
def test_i8_graph_index_is_the_f32_graph_index_over_decoded_rows(metric, tmp_path):
    import torch
    from annlite_amd import HnswFlatGpuIndex
    from annlite_amd.enums import Metric

    torch.cuda.set_device(0)
    metric = Metric[metric]
    s = 2.0 ** -4 if metric == Metric.EUCLIDEAN else 2.0 ** -7  # (COSINE: the parent's default)
    rs = np.random.RandomState(5)
    centres = 2.0 * rs.randn(40, D).astype(np.float32)
    codes = np.clip(np.rint((rs.randn(N, D).astype(np.float32) + centres[rs.randint(0, 40, N)]) / 2.0 ** -4), -127, 127)
    x = (2.0 ** -4 * codes).astype(np.float32)  # (EUCLIDEAN: rows the int8 index stores exactly)
    q = rs.randn(B, D).astype(np.float32) + centres[rs.randint(0, 40, B)]
    q[0] = x[123]
    some = np.nonzero(rs.rand(N) < 0.5)[0]
    new = lambda rows, **kw: HnswFlatGpuIndex(D, metric=metric, graph_rows=rows, **kw, **KNOBS)
    new8 = lambda: new('i8', **(dict(int8_scale=s) if metric == Metric.EUCLIDEAN else {}))
    h8, h32 = new8(), new('f32')
    for idx in (h8, h32):
        idx.add_with_ids(x[:9000], np.arange(9000))
        idx.add_with_ids(x[9000:], np.arange(9000, N))
    assert h8.graph_rows == 'i8' and h8.int8_scale_ == s and h8._vectors.dtype == torch.int8 and h32._vectors.dtype == torch.float32
    if metric == Metric.COSINE:  # (module docstring)
        h32._vectors[:N] = s * h8._vectors[:N].float()
        h32._kind.norms(h32._vectors, n=N, out=h32._norms)
        h8._rebuild_graph(N)
        h32._rebuild_graph(N)
    assert torch.equal(s * h8._vectors[:N].float(), h32._vectors[:N])
    assert h8._gg.n == N and torch.equal(h8._gg.links[:N], h32._gg.links[:N])
    got = h8.search_batch(q, limit=K, ef_search=EF)
    assert _same(got, h32.search_batch(q, limit=K, ef_search=EF))
    if metric == Metric.EUCLIDEAN:
        assert got[1][0][0] == 123 and got[0][0][0] == 0.0  # a stored row finds itself at 0.0
    fgot = h8.search_batch(q, limit=K, ef_search=EF, indices=some, filter_search='graph')
    assert h8.last_filter_path == 'graph'
    assert _same(fgot, h32.search_batch(q, limit=K, ef_search=EF, indices=some, filter_search='graph'))
    assert np.isin(fgot[1][fgot[1] >= 0], some).all()
    # dump -> load: the same links and answers
    h8.dump(tmp_path / 'h8.idx')
    again = new8()
    again.load(tmp_path / 'h8.idx')
    assert torch.equal(again._gg.links[:N], h8._gg.links[:N]) and _same(again.search_batch(q, limit=K, ef_search=EF), got)
    # an f32 graph index's file: rows converted, links dropped, the graph rebuilt -- an int8 index linked from nothing over those rows
    h32.dump(tmp_path / 'h32.idx')
    conv = new8()
    conv.load(tmp_path / 'h32.idx')
    assert conv._vectors.dtype == torch.int8 and conv._gg.n == N and torch.equal(conv._vectors[:N], h8._vectors[:N])
    if metric == Metric.EUCLIDEAN:
        assert not torch.equal(conv._gg.links[:N], h32._gg.links[:N])  # (not the file's links: those came from two calls)
        h8._rebuild_graph(N)
    assert torch.equal(conv._gg.links[:N], h8._gg.links[:N])
    assert _same(conv.search_batch(q, limit=K, ef_search=EF), h8.search_batch(q, limit=K, ef_search=EF))


def test_graph_rows_i8_keyword(tmp_path):
    from annlite_amd import AnnLite, HnswFlatGpuIndex

    ann = AnnLite(D, metric='euclidean', graph=True, build='gpu', graph_rows='i8', int8_scale=0.25, data_path=tmp_path / 'g')
    idx = ann.vec_index(0)
    assert type(idx) is HnswFlatGpuIndex and idx.graph_rows == 'i8' and idx.int8_scale_ == 0.25
    with pytest.raises(NotImplementedError, match="graph_rows='i8'"):
        HnswFlatGpuIndex(D, dtype=np.int8)
    with pytest.raises(ValueError, match='int8_scale'):
        HnswFlatGpuIndex(D, graph_rows='f16', int8_scale=0.25)
