"""CPU: ``ivf_rows='i8'`` of ``IvfFlatGpuIndex`` and of the facade (no device work: nothing is allocated before the first rows)."""
import numpy as np
import pytest


def test_ivf_rows_i8_keyword_refusals_and_facade(tmp_path):
    import torch
    from annlite_amd import AnnLite
    from annlite_amd.core.codec.vq import VQCodec
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex
    from annlite_amd.enums import Metric

    vq = VQCodec(4)
    idx = IvfFlatGpuIndex(8, vq_codec=vq, n_probe=2, ivf_rows='i8')
    assert idx.ivf_rows == 'i8' and idx._i8 and not idx._f16 and idx.flat_filter == 'i8x3' and idx.last_cell_filter is None
    assert idx._columns()['_vectors'] == ((8,), torch.int8) and idx._columns()['_cell_of'] == ((), torch.int32)
    assert idx.int8_scale_ == 2.0 ** -7  # the defaults: 2^-7 for COSINE (the constructor's metric), 1.0 for the others
    assert IvfFlatGpuIndex(8, vq_codec=vq, metric=Metric.EUCLIDEAN, ivf_rows='i8').int8_scale_ == 1.0
    assert IvfFlatGpuIndex(8, vq_codec=vq, ivf_rows='i8', int8_scale=0.125, dtype=np.int8).int8_scale_ == 0.125
    for kw, match in ((dict(cell_filter='bf16x3'), "ivf_rows='i8'"), (dict(centre=None), "ivf_rows='i8'"), (dict(dim=32769), '32768'),
                      (dict(int8_scale=3.0), 'int8_scale'), (dict(int8_scale=2.0 ** 25), 'int8_scale')):
        with pytest.raises(ValueError, match=match):
            IvfFlatGpuIndex(**{'dim': 8, 'vq_codec': vq, 'ivf_rows': 'i8', **kw})
    with pytest.raises(ValueError, match='int8_scale'):  # the scale of int8 rows: not with the other row kinds
        IvfFlatGpuIndex(8, vq_codec=vq, ivf_rows='f16', int8_scale=0.5)
    with pytest.raises(NotImplementedError, match="int8.*ivf_rows='i8'"):  # without the keyword: refused as before, and the way in is named
        IvfFlatGpuIndex(8, vq_codec=vq, dtype=np.int8)
    # the facade: an IvfFlatGpuIndex over int8 rows, the scale through the same channel ...
    idx = AnnLite(16, n_cells=4, n_probe=2, ivf_prune=True, ivf_rows='i8', int8_scale=2.0 ** -3, data_path=tmp_path / 'a').vec_index(0)
    assert type(idx) is IvfFlatGpuIndex and idx.ivf_rows == 'i8' and idx.int8_scale_ == 0.125
    assert idx._columns()['_vectors'] == ((16,), torch.int8)
    # ... and both keywords dropped by an index over PQ codes
    AnnLite(16, n_subvectors=4, n_cells=4, ivf_rows='i8', int8_scale=0.5, data_path=tmp_path / 'b')
