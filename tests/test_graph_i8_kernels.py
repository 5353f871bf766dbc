"""The float graph over INT8 rows (graph_i8.hip) pinned BIT FOR BIT.  The walk (annlite_graph_i8_search): against the restated walk
order of tests/_refs.py over ``ops.exact_gather_dist_i8`` of all rows -- the bits every distance of the int8 graph carries --, against
``ops.graph_f32_search`` over the rows ``scale * code``, and against float64 within the fp32 summation bound.  The admit walk and the
two build kernels: against their f32 twins over the decoded rows (pinned to restatements by the f32 graph's own tests; decoding a code
is exact, so equality with the twin is the sharp check).

The shapes are the ones at which the eighth-wave distance (8 lanes per row, eight chains per lane, eight rows per pass) can go wrong:
one active lane of a group (D = 8), a tail block that ends inside a group (D = 56), one that crosses 64 (D = 72, 200), partial passes
(L = 5, 17), more rows than one set of passes holds (L = 64), D = 2048, and the lane-strided path of every D % 8 != 0 (D = 1, 3, 4, 60,
130; 4 and 60 are the quarter-wave variant's edges)."""
import numpy as np
import pytest

from _refs import bitmap, f32_key, fp32_chain_bound, random_links, walk_restated
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason='needs a GPU')]

EUCLIDEAN, INNER_PRODUCT, COSINE = 1, 2, 3
N, B, N_SEEDS = 3000, 10, 150


@pytest.fixture(scope='module')
def ops():
    import torch
    from annlite_amd import ops as _ops

    torch.cuda.set_device(0)
    return _ops


def _codes(rs, n, D):
    x = np.clip(np.rint(40.0 * rs.randn(n, D)), -127, 127).astype(np.int8)
    x[1000:1040] = x[1000]  # exact ties inside the walk: the node id decides
    x[5] = np.where(np.arange(D) % 2, -127, 127)
    x[6] = 0
    return x


@pytest.mark.parametrize('metric,D,L,ef,scale', [(EUCLIDEAN, *s, 2.0 ** -5) for s in [
    (128, 32, 128), (64, 32, 64), (8, 5, 10), (56, 17, 33), (72, 17, 33), (200, 32, 129), (768, 24, 256), (2048, 8, 32), (128, 64, 100),
    (1, 4, 8), (3, 5, 10), (4, 5, 10), (60, 17, 33), (130, 32, 64)]] + [
    (INNER_PRODUCT, 128, 32, 128, 2.0 ** -5), (INNER_PRODUCT, 64, 32, 64, 2.0 ** -5), (COSINE, 128, 32, 128, 2.0 ** -5),
    (COSINE, 64, 32, 64, 2.0 ** -5), (EUCLIDEAN, 128, 32, 128, 1.0)])
def test_i8_walk_equals_restatement_gather_and_f32_twin(ops, metric, D, L, ef, scale):
    import torch

    rs = np.random.RandomState(metric * 100003 + D * 1000 + L * 7)
    links, x = random_links(rs, N, L), _codes(rs, N, D)
    q = (scale * 40.0 * rs.randn(B, D)).astype(np.float32)
    q[2] = scale * x[77].astype(np.float32)  # a stored row as its own query
    q[4, D // 2] = np.nan
    q[7, 0] = np.inf
    seeds = rs.choice(N, N_SEEDS, replace=False).astype(np.int32)
    if 77 not in seeds:
        seeds[0] = 77  # (random links are no proximity graph: the row that is its own query is a seed)
    valid = rs.rand(N) < 0.9
    x_d, q_d, links_d, seeds_d = ops.to_dev(x), ops.to_dev(q), ops.to_dev(links), ops.to_dev(seeds)
    xf_d = scale * x_d.float()
    all_rows = torch.arange(N, device='cuda', dtype=torch.int64)[None, :].expand(B, N).contiguous()
    keys = f32_key(ops.exact_gather_dist_i8(metric, q_d, x_d, all_rows, scale).cpu().numpy())
    lk = links.view(np.uint32)
    for vbits, vmask in ((ops.to_dev(bitmap(valid)), valid), (None, None)):
        gi, gd = ops.graph_i8_search(metric, q_d, x_d, links_d, seeds_d, ef, valid_bits=vbits, scale=scale)
        fi, fd = ops.graph_f32_search(metric, q_d, xf_d, links_d, seeds_d, ef, valid_bits=vbits)
        torch.cuda.synchronize()
        gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
        for b in range(B):
            ri, rbits = walk_restated(lk, seeds, keys[b], ef, vmask)
            assert np.array_equal(gi[b], ri), (vmask is not None, b)
            assert np.array_equal(gd[b].view(np.uint32), rbits), (vmask is not None, b)
        assert np.array_equal(gi, fi.cpu().numpy()) and np.array_equal(gd.view(np.uint32), fd.cpu().numpy().view(np.uint32))
    # (gi, gd: the walk without the bitmap -- under it row 77 may be blanked)
    if metric == EUCLIDEAN:
        assert gi[2, 0] == 77 and gd[2, 0].view(np.uint32) == 0  # +0.0
    if D in (8, 768, 2048):
        x64 = scale * x.astype(np.float64)
        for b in range(B):
            ok = (gi[b] >= 0) & np.isfinite(gd[b])
            terms = (x64[gi[b][ok]] - q[b].astype(np.float64)) ** 2 if metric == EUCLIDEAN else x64[gi[b][ok]] * q[b].astype(np.float64)
            d64 = terms.sum(1) if metric == EUCLIDEAN else 1.0 - terms.sum(1)
            assert (np.abs(gd[b][ok].astype(np.float64) - d64) <= fp32_chain_bound(terms, d64, D)).all(), b


@pytest.mark.parametrize('metric', [EUCLIDEAN, INNER_PRODUCT])
@pytest.mark.parametrize('D,L', [(128, 32), (56, 17)])
def test_i8_admit_walk_select_and_reverse_equal_their_f32_twins(ops, metric, D, L):
    import torch

    scale, n, b, ef = 2.0 ** -5, 2000, 37, 96
    rs = np.random.RandomState(metric * 1009 + D)
    x_d = ops.to_dev(_codes(rs, n, D))
    xf_d = scale * x_d.float()
    # the admit walk
    links_d = ops.to_dev(random_links(rs, n, L))
    seeds_d = ops.to_dev(rs.choice(n, 150, replace=False).astype(np.int32))
    q_d = torch.cat([ops.to_dev((scale * 40.0 * rs.randn(9, D)).astype(np.float32)), xf_d[77:78]])
    admit = ops.to_dev(bitmap(rs.rand(n) < 0.3))
    worst = torch.empty((2, 10), dtype=torch.float32, device='cuda')
    gi, gd = ops.graph_i8_search_admit(metric, q_d, x_d, links_d, seeds_d, 128, 64, admit, route_worst=worst[0], scale=scale)
    wi, wd = ops.graph_f32_search_admit(metric, q_d, xf_d, links_d, seeds_d, 128, 64, admit, route_worst=worst[1])
    assert torch.equal(gi, wi) and torch.equal(gd.view(torch.int32), wd.view(torch.int32))
    assert torch.equal(worst[0].view(torch.int32), worst[1].view(torch.int32)) and int((wi >= 0).sum()) > 10 * 32
    # select: random candidate lists longer than `keep`, with the base point, ids beyond the table and holes among them
    base0 = n - b
    cand = rs.randint(0, base0, (b, ef)).astype(np.int64)
    cand[:, 5], cand[:, 9], cand[:, 11], cand[::3, 40:], cand[1, 6:] = base0 + np.arange(b), n + 5, -1, -1, -1  # (row 1: a pool that fits)
    cand_d = ops.to_dev(cand)
    got_links, want_links = (torch.zeros((n, L + 1), dtype=torch.int32, device='cuda') for _ in range(2))
    got = ops.graph_i8_build_select(metric, cand_d, base0, x_d, L // 2, got_links, scale=scale)
    want = ops.graph_f32_build_select(metric, cand_d, base0, xf_d, L // 2, want_links)
    assert torch.equal(got, want) and torch.equal(got_links, want_links) and int(want_links[base0:, 0].max()) >= 2
    # reverse: full lists of 120 targets meet 1 .. 40 sources each -- appended where there is room, shrunk by the heuristic elsewhere
    half = n // 2
    links = np.zeros((n, L + 1), np.uint32)
    pairs = []
    for t_i, t in enumerate(rs.choice(half, 120, replace=False)):
        c = [0, L // 2, L, L][t_i % 4]
        links[t, 0], links[t, 1:1 + c] = c, rs.choice(np.setdiff1d(np.arange(half), [t]), c, replace=False)
        pairs += [(int(t) << 32) | int(s) for s in rs.choice(np.arange(half, n), [1, 3, 12, 40][(t_i // 4) % 4], replace=False)]
    keys = np.array(sorted(pairs), dtype=np.int64)
    seg = np.concatenate([[0], np.nonzero(np.diff(keys >> 32))[0] + 1, [len(keys)]]).astype(np.int64)
    keys_d, seg_d = ops.to_dev(keys), ops.to_dev(seg)
    got, want = ops.to_dev(links.view(np.int32)), ops.to_dev(links.view(np.int32))
    ops.graph_i8_build_reverse(metric, keys_d, seg_d, x_d, got, scale=scale)
    ops.graph_f32_build_reverse(metric, keys_d, seg_d, xf_d, want)
    assert torch.equal(got, want) and not torch.equal(want, ops.to_dev(links.view(np.int32)))
