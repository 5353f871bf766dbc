"""``HnswFlatGpuIndex(graph_rows='f16')``: the float graph over half-precision rows is, bit for bit, the f32 graph index over the same
rows rounded to f16 -- same links, same ids, same distance bits, with and without a filter answered on the graph -- at half the row
bytes.  N = 12000 lies above ``BRUTE`` (8192): batches fed by the f16 walk are built.

COSINE: an f32 index normalises what it is fed, so feeding it rounded rows does not leave it the f16 index's rows (those are normalised
first, then rounded).  There the f32 twin's rows are overwritten with the f16 index's, widened, and BOTH graphs are linked again from
nothing (``_rebuild_graph``: 8192 rows by exact lists, two batches fed by the walk)."""
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
def test_f16_graph_index_is_the_f32_graph_index_over_rounded_rows(metric, tmp_path):
    import torch
    from annlite_amd import HnswFlatGpuIndex
    from annlite_amd.enums import Metric

    torch.cuda.set_device(0)
    metric = Metric[metric]
    rs = np.random.RandomState(5)
    centres = 2.0 * rs.randn(40, D).astype(np.float32)
    x16 = (rs.randn(N, D).astype(np.float32) + centres[rs.randint(0, 40, N)]).astype(np.float16)
    q = rs.randn(B, D).astype(np.float32) + centres[rs.randint(0, 40, B)]
    q[0] = x16[123].astype(np.float32)
    some = np.nonzero(rs.rand(N) < 0.5)[0]
    new = lambda rows: HnswFlatGpuIndex(D, metric=metric, graph_rows=rows, **KNOBS)
    h16, h32 = new('f16'), new('f32')
    for idx in (h16, h32):
        idx.add_with_ids(x16[:9000].astype(np.float32), np.arange(9000))
        idx.add_with_ids(x16[9000:].astype(np.float32), np.arange(9000, N))
    assert h16.graph_rows == 'f16' and h32.graph_rows == 'f32'
    assert h16._vectors.dtype == torch.float16 and h32._vectors.dtype == torch.float32
    if metric == Metric.COSINE:  # (module docstring)
        h32._vectors[:N] = h16._vectors[:N].float()
        h32._kind.norms(h32._vectors, n=N, out=h32._norms)
        h16._rebuild_graph(N)
        h32._rebuild_graph(N)
    assert torch.equal(h16._vectors[:N].float(), h32._vectors[:N])
    assert h16._gg.n == N and torch.equal(h16._gg.links[:N], h32._gg.links[:N])
    got = h16.search_batch(q, limit=K, ef_search=EF)
    assert _same(got, h32.search_batch(q, limit=K, ef_search=EF))
    if metric == Metric.EUCLIDEAN:
        assert got[1][0][0] == 123 and got[0][0][0] == 0.0  # a stored row finds itself at 0.0
    fgot = h16.search_batch(q, limit=K, ef_search=EF, indices=some, filter_search='graph')
    assert h16.last_filter_path == 'graph'
    assert _same(fgot, h32.search_batch(q, limit=K, ef_search=EF, indices=some, filter_search='graph'))
    assert np.isin(fgot[1][fgot[1] >= 0], some).all()
    # dump -> load: the same links and answers
    h16.dump(tmp_path / 'h16.idx')
    again = new('f16')
    again.load(tmp_path / 'h16.idx')
    assert torch.equal(again._gg.links[:N], h16._gg.links[:N]) and _same(again.search_batch(q, limit=K, ef_search=EF), got)
    # an f32 graph index's file: rows converted, links dropped, the graph rebuilt -- an f16 index built from those rows in one call
    h32.dump(tmp_path / 'h32.idx')
    conv = new('f16')
    conv.load(tmp_path / 'h32.idx')
    assert conv._vectors.dtype == torch.float16 and conv._gg.n == N
    if metric == Metric.EUCLIDEAN:
        built = new('f16')
        built.add_with_ids(x16.astype(np.float32), np.arange(N))
        assert not torch.equal(conv._gg.links[:N], h32._gg.links[:N])  # (not the file's links: those came from two calls)
    else:
        built = h16  # (linked from nothing above, over these very rows)
    assert torch.equal(conv._gg.links[:N], built._gg.links[:N])
    assert _same(conv.search_batch(q, limit=K, ef_search=EF), built.search_batch(q, limit=K, ef_search=EF))


def test_graph_rows_keyword(tmp_path):
    from annlite_amd import AnnLite, HnswFlatGpuIndex

    ann = AnnLite(D, metric='euclidean', graph=True, build='gpu', graph_rows='f16', data_path=tmp_path / 'g')
    idx = ann.vec_index(0)
    assert type(idx) is HnswFlatGpuIndex and idx.graph_rows == 'f16'
    with pytest.raises(ValueError, match='graph_rows'):
        HnswFlatGpuIndex(D, graph_rows='f64')
    with pytest.raises(NotImplementedError, match='float16'):
        HnswFlatGpuIndex(D, dtype=np.float16)
    with pytest.raises(NotImplementedError, match='int8'):
        HnswFlatGpuIndex(D, dtype=np.int8, graph_rows='f16')
