"""CPU: the ``ivf_rows`` keyword of ``IvfFlatGpuIndex`` and of the facade (no device work: nothing is allocated before the first rows)."""
import numpy as np
import pytest


def test_ivf_rows_keyword_refusals_and_facade(tmp_path):
    import torch
    from annlite_amd import AnnLite
    from annlite_amd.core.codec.vq import VQCodec
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.core.index.hnsw_flat_gpu import HnswFlatGpuIndex
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex

    vq = VQCodec(4)
    idx, plain = IvfFlatGpuIndex(8, vq_codec=vq, n_probe=2, ivf_rows='f16'), IvfFlatGpuIndex(8, vq_codec=vq)
    assert idx.ivf_rows == 'f16' and idx._f16 and idx.flat_filter == 'f16x2' and idx.last_cell_filter is None
    assert idx._columns()['_vectors'] == ((8,), torch.float16) and idx._columns()['_cell_of'] == ((), torch.int32)
    assert plain.ivf_rows == 'f32' and not plain._f16 and plain._columns()['_vectors'] == ((8,), torch.float32)
    raw = torch.tensor([[1.0002, 70000.0]])
    assert torch.equal(plain._cell_vectors(raw), raw)  # the f32 index assigns its cells from the vectors as given ...
    assert idx._cell_vectors(raw).tolist() == [[1.0, float('inf')]]  # ... the f16 index from the vectors as it rounds them
    for kw, match in ((dict(ivf_rows='f64'), 'ivf_rows'), (dict(ivf_rows=None), 'ivf_rows'), (dict(cell_filter='bf16x3'), "ivf_rows='f16'"),
                      (dict(centre=None), "ivf_rows='f16'"), (dict(centre=np.zeros(8, np.float32)), "ivf_rows='f16'"), (dict(dim=32769), '32768')):
        with pytest.raises(ValueError, match=match):
            IvfFlatGpuIndex(**{'dim': 8, 'vq_codec': vq, 'ivf_rows': 'f16', **kw})
    with pytest.raises(NotImplementedError, match="float16.*ivf_rows='f16'"):  # without the keyword: refused as before, and the way in is named
        IvfFlatGpuIndex(8, vq_codec=vq, dtype=np.float16)
    for kw in (dict(), dict(ivf_rows='f16')):
        with pytest.raises(NotImplementedError, match='int8'):
            IvfFlatGpuIndex(8, vq_codec=vq, dtype=np.int8, **kw)
    # the facade: an IvfFlatGpuIndex over f16 rows ...
    idx = AnnLite(16, n_cells=4, n_probe=2, ivf_prune=True, ivf_rows='f16', data_path=tmp_path / 'a').vec_index(0)
    assert type(idx) is IvfFlatGpuIndex and idx.ivf_rows == 'f16' and idx._columns()['_vectors'] == ((16,), torch.float16)
    assert AnnLite(16, n_cells=4, ivf_prune=True, data_path=tmp_path / 'b').vec_index(0).ivf_rows == 'f32'
    with pytest.raises(ValueError, match='ivf_rows'):
        AnnLite(16, n_cells=4, ivf_prune=True, ivf_rows='half', data_path=tmp_path / 'c')
    # ... and the keyword swallowed where none is built: the plain flat index, the float graph, everything over PQ codes
    flat = AnnLite(16, ivf_rows='f16', data_path=tmp_path / 'd').vec_index(0)
    assert type(flat) is FlatGpuIndex and not flat._f16
    assert type(AnnLite(16, graph=True, build='gpu', ivf_rows='f16', data_path=tmp_path / 'e').vec_index(0)) is HnswFlatGpuIndex
    for n, kw in enumerate((dict(), dict(n_cells=4), dict(graph=True))):
        AnnLite(16, n_subvectors=4, ivf_rows='f16', data_path=tmp_path / f'f{n}', **kw)
