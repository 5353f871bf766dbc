#!/usr/bin/env python3
"""The float HNSW graph (HnswFlatGpuIndex): build time, queries/s and recall@10 against exact search at
ef_search 64 / 128 / 192 on one and two caller streams, FlatGpuIndex on the same table, and the walk's row-gather rate.

    python scripts/bench_hnsw_flat.py --rows 1000000        # one JSON line on stdout
    python scripts/bench_hnsw_flat.py --rows 1000000 --graph-rows both

``--graph-rows f16``: the graph over half-precision rows (``graph_rows='f16'``).  ``both``: an f32 and an f16 index over the SAME data
rounded to f16 -- the f32 index stores the rounded values, so both graphs, all answers and all counters are identical (checked); the two
indexes alternate inside every measurement, in one process, and each one's figures are reported side by side under ``f32`` / ``f16``.

``--graph-rows i8``: the graph over int8 rows (``graph_rows='i8'``, int8_scale 1.0: give the data a ``--data-scale``).  ``all``: an f32,
an f16 and an int8 index over the SAME data rounded to whole code steps in [-127, 127] -- values all three store exactly --, checked and
measured like ``both``, under ``f32`` / ``f16`` / ``i8``.  ``--data-scale S``: rows and queries are scaled so that a coordinate's
standard deviation is S code steps.  With ``i8`` / ``all`` recall@10 is against the exact search over the UNROUNDED rows.

Data: scripts/bench_hnsw.py's generator (a 16-d latent mixed into D dimensions + noise, the same seeds), EUCLIDEAN.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from annlite_amd import HnswFlatGpuIndex, Metric, _capi, ops  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--rows', type=int, default=1_000_000)
p.add_argument('--dim', type=int, default=128)
p.add_argument('--batch', type=int, default=1024)
p.add_argument('--k', type=int, default=10)
p.add_argument('--ef-search', type=int, nargs='+', default=[64, 128, 192])
p.add_argument('--ef-construction', type=int, default=200)
p.add_argument('--max-connection', type=int, default=16)
p.add_argument('--steps', type=int, default=5)
p.add_argument('--graph-rows', choices=['f32', 'f16', 'i8', 'both', 'all'], default='f32')
p.add_argument('--data-scale', type=float, default=None, help="a coordinate's standard deviation in int8 code steps (default: unscaled)")
a = p.parse_args()
dev = torch.device('cuda', 0)
torch.cuda.set_device(0)
N, D, B, k = a.rows, a.dim, a.batch, a.k
r_lat = 16 if D <= 128 else 64
g = torch.Generator(device=dev)
g.manual_seed(99)
A = torch.randn((r_lat, D), generator=g, device=dev)
CH = 250_000
MUL = 1.0 if a.data_scale is None else a.data_scale / (r_lat + 0.0025) ** 0.5  # (a coordinate of z @ A + 0.05 e has variance r_lat + 0.0025)


def gen(chunk, rows, rounded=True):
    gg = torch.Generator(device=dev)
    gg.manual_seed(1234 + chunk)
    z = torch.randn((rows, r_lat), generator=gg, device=dev)
    e = torch.randn((rows, D), generator=gg, device=dev)
    x = ((z @ A + 0.05 * e) * MUL).contiguous()
    if rounded and a.graph_rows == 'all':
        return torch.round(x).clamp_(-127.0, 127.0)
    return x.half().float() if rounded and a.graph_rows == 'both' else x


def queries(seed):
    gq = torch.Generator(device=dev)
    gq.manual_seed(seed)
    return ((torch.randn((B, r_lat), generator=gq, device=dev) @ A + 0.05 * torch.randn((B, D), generator=gq, device=dev)) * MUL).contiguous()


kinds = {'both': ['f32', 'f16'], 'all': ['f32', 'f16', 'i8']}.get(a.graph_rows, [a.graph_rows])
indexes, build_s = {}, {}
for kind in kinds:
    index = HnswFlatGpuIndex(D, metric=Metric.EUCLIDEAN, initial_size=N, ef_search=a.ef_search[0], ef_construction=a.ef_construction,
                             max_connection=a.max_connection, graph_rows=kind)
    torch.cuda.synchronize()
    t0 = time.time()
    for c in range((N + CH - 1) // CH):
        rows = min(CH, N - c * CH)
        index.add_with_ids(gen(c, rows), torch.arange(c * CH, c * CH + rows, device=dev, dtype=torch.int64))
    torch.cuda.synchronize()
    indexes[kind], build_s[kind] = index, time.time() - t0
index = indexes[kinds[0]]
for kind in kinds[1:]:
    assert torch.equal(index._gg.links[:N], indexes[kind]._gg.links[:N]), f'the {kinds[0]} and the {kind} graph differ'

q, q_alt = queries(4321), queries(4321 + 7919)
q_rot = [q, q_alt]  # the timed steps rotate through two query batches (recall is the first batch's)
side = [torch.cuda.Stream(device=dev) for _ in range(2)]
# exact truth: the index's own exhaustive search (FlatGpuIndex.search_batch on the same rows); with int8 rows: over the UNROUNDED rows
if 'i8' in kinds:
    best_d, best_i = torch.full((B, k), float('inf'), device=dev), torch.full((B, k), -1, device=dev, dtype=torch.int64)
    for c in range((N + CH - 1) // CH):
        d, i = torch.topk(torch.cdist(q, gen(c, min(CH, N - c * CH), rounded=False)), k, dim=1, largest=False)
        best_d, pick = torch.topk(torch.cat([best_d, d], 1), k, dim=1, largest=False)
        best_i = torch.gather(torch.cat([best_i, i + c * CH], 1), 1, pick)
    truth = best_i.cpu().numpy()
else:
    truth = index.search_exhaustive(q, limit=k)[1].cpu().numpy()


def recall(ids):
    ids = ids.cpu().numpy()
    return float(np.mean([len(set(ids[b]) & set(truth[b])) / k for b in range(B)]))


def timed(fn, streams=1):
    """fn(batch) -> result; `streams` > 1: consecutive batches on alternating caller streams."""
    for j in range(4):  # (warm-up ON the streams that are timed: torch's allocator keeps a pool per stream)
        with torch.cuda.stream(side[j % streams] if streams > 1 else torch.cuda.current_stream()):
            fn(q_rot[j % 2])
    torch.cuda.synchronize()
    n = max(a.steps, 2)
    t = time.perf_counter()
    if streams > 1:
        for j in range(n):
            with torch.cuda.stream(side[j % streams]):
                fn(q_rot[j % 2])
    else:
        for j in range(n):
            fn(q_rot[j % 2])
    torch.cuda.synchronize()
    el = time.perf_counter() - t
    out = fn(q)
    torch.cuda.synchronize()
    return out, B * n / el


def walk_ms(qd, ef):
    """{kind: mean ms of the walk kernel by HIP events}; the indexes alternate launch by launch"""
    for _ in range(2):
        for kind in kinds:
            indexes[kind].candidates(qd, ef)
    torch.cuda.synchronize()
    out = {kind: [] for kind in kinds}
    for _ in range(max(3, a.steps)):
        for kind in kinds:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            indexes[kind].candidates(qd, ef)
            e1.record()
            e1.synchronize()
            out[kind].append(e0.elapsed_time(e1))
    return {kind: float(np.mean(v)) for kind, v in out.items()}


def counters(idx, qd, ef):
    os.environ['ANNLITE_DEBUG_COUNTERS'] = '1'
    _capi.knobs_reload()  # (the library parses its switches at load)
    idx.candidates(qd, ef)
    out = ops.graph_f32_search_stats()
    del os.environ['ANNLITE_DEBUG_COUNTERS']
    _capi.knobs_reload()
    return out


qd = index._pre(q)
lpn = 2 * a.max_connection
n_seeds = int(index._gg.seeds().numel())
res = {kind: {} for kind in kinds}
for ef in a.ef_search:
    qps, ans, cnt = {kind: [None, None] for kind in kinds}, {}, {}
    for rep_ in range(2):  # (the indexes alternate: one stream, then two, each index in turn)
        for kind in kinds:
            search = lambda qq, idx=indexes[kind]: idx.search_batch(qq, limit=k, ef_search=ef)
            ans[kind], qps[kind][rep_] = timed(search, 1 + rep_)
    for kind in kinds:
        cnt[kind] = counters(indexes[kind], qd, ef)
    ms = walk_ms(qd, ef)
    for kind in kinds[1:]:
        assert cnt[kinds[0]] == cnt[kind], ('the walks counted differently', cnt)
        assert all(torch.equal(u, v) for u, v in zip(ans[kinds[0]], ans[kind])), f'the {kinds[0]} and the {kind} index answer differently'
    for kind in kinds:
        n_expand, n_eval = cnt[kind]
        row_bytes = n_eval * D * float(indexes[kind]._vectors.element_size())  # the gathered rows (seed rows included)
        list_bytes = n_expand * 4.0 * (lpn + 1)                                # one link list per expansion
        res[kind][f'ef_search_{ef}'] = {'queries_per_s_one_stream': qps[kind][0], 'queries_per_s_two_streams': qps[kind][1],
                                        'recall_at_10': recall(ans[kind][1]), 'walk_kernel_ms': ms[kind],
                                        'expansions_per_query': n_expand / B, 'rows_evaluated_per_query': n_eval / B,
                                        'row_gather_GBps': row_bytes / (ms[kind] * 1e-3) / 1e9,
                                        'row_and_list_GBps': (row_bytes + list_bytes) / (ms[kind] * 1e-3) / 1e9}

# FlatGpuIndex on the same table: the index's own exhaustive search (its parent's search_batch over the same rows)
(fd, fi), flat_qps1 = timed(lambda qq: index.search_exhaustive(qq, limit=k), 1)
_, flat_qps2 = timed(lambda qq: index.search_exhaustive(qq, limit=k), 2)

links = index._gg.links[:N, 0].float()
first = res[kinds[0]][f'ef_search_{a.ef_search[0]}']
per_kind = {kind: {'build_s': build_s[kind], 'build_rows_per_s': N / build_s[kind],
                   'row_column_bytes': N * D * indexes[kind]._vectors.element_size(), **res[kind]} for kind in kinds}
print(json.dumps({'config': f'float HNSW (level 0, GPU-built): {N} x {D}-dim, graph rows {a.graph_rows}, L2, '
                            f'max_connection={a.max_connection}, ef_construction={a.ef_construction}, batch {B}, k={k}, {n_seeds} seeds',
                  'metric': 'queries/sec', 'unit': 'queries/s', 'value': first['queries_per_s_two_streams'],
                  'recall_at_10': first['recall_at_10'], 'mean_links_per_node': float(links.mean().item()),
                  'flat_exact_queries_per_s_one_stream': flat_qps1, 'flat_exact_queries_per_s_two_streams': flat_qps2,
                  'steps': max(a.steps, 2), 'query_batches': 2, **(per_kind if len(kinds) > 1 else per_kind[kinds[0]])}))
