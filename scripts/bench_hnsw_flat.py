#!/usr/bin/env python3
"""The float HNSW graph (HnswFlatGpuIndex): build time, queries/s and recall@10 against exact search at
ef_search 64 / 128 / 192 on one and two caller streams, FlatGpuIndex on the same table, and the walk's row-gather rate.

    python scripts/bench_hnsw_flat.py --rows 1000000        # one JSON line on stdout

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
a = p.parse_args()
dev = torch.device('cuda', 0)
torch.cuda.set_device(0)
N, D, B, k = a.rows, a.dim, a.batch, a.k
r_lat = 16 if D <= 128 else 64
g = torch.Generator(device=dev)
g.manual_seed(99)
A = torch.randn((r_lat, D), generator=g, device=dev)
CH = 250_000


def gen(chunk, rows):
    gg = torch.Generator(device=dev)
    gg.manual_seed(1234 + chunk)
    z = torch.randn((rows, r_lat), generator=gg, device=dev)
    e = torch.randn((rows, D), generator=gg, device=dev)
    return (z @ A + 0.05 * e).contiguous()


def queries(seed):
    gq = torch.Generator(device=dev)
    gq.manual_seed(seed)
    return (torch.randn((B, r_lat), generator=gq, device=dev) @ A + 0.05 * torch.randn((B, D), generator=gq, device=dev)).contiguous()


index = HnswFlatGpuIndex(D, metric=Metric.EUCLIDEAN, initial_size=N, ef_search=a.ef_search[0], ef_construction=a.ef_construction,
                         max_connection=a.max_connection)
torch.cuda.synchronize()
t0 = time.time()
for c in range((N + CH - 1) // CH):
    rows = min(CH, N - c * CH)
    index.add_with_ids(gen(c, rows), torch.arange(c * CH, c * CH + rows, device=dev, dtype=torch.int64))
torch.cuda.synchronize()
build_s = time.time() - t0

q, q_alt = queries(4321), queries(4321 + 7919)
q_rot = [q, q_alt]  # the timed steps rotate through two query batches (recall is the first batch's)
side = [torch.cuda.Stream(device=dev) for _ in range(2)]
# exact truth: the index's own exhaustive search (FlatGpuIndex.search_batch on the same rows)
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
    for _ in range(2):
        index.candidates(qd, ef)
    torch.cuda.synchronize()
    out = []
    for _ in range(max(3, a.steps)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        index.candidates(qd, ef)
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.mean(out))


qd = index._pre(q)
lpn = 2 * a.max_connection
n_seeds = int(index._gg.seeds().numel())
res = {}
for ef in a.ef_search:
    (d, i), qps1 = timed(lambda qq: index.search_batch(qq, limit=k, ef_search=ef), 1)
    _, qps2 = timed(lambda qq: index.search_batch(qq, limit=k, ef_search=ef), 2)
    os.environ['ANNLITE_DEBUG_COUNTERS'] = '1'
    _capi.knobs_reload()  # (the library parses its switches at load)
    index.candidates(qd, ef)
    n_expand, n_eval = ops.graph_f32_search_stats()
    del os.environ['ANNLITE_DEBUG_COUNTERS']
    _capi.knobs_reload()
    ms = walk_ms(qd, ef)
    row_bytes = n_eval * D * 4.0                # the gathered rows (seed rows included)
    list_bytes = n_expand * 4.0 * (lpn + 1)     # one link list per expansion
    res[f'ef_search_{ef}'] = {'queries_per_s_one_stream': qps1, 'queries_per_s_two_streams': qps2, 'recall_at_10': recall(i),
                              'walk_kernel_ms': ms, 'expansions_per_query': n_expand / B, 'rows_evaluated_per_query': n_eval / B,
                              'row_gather_GBps': row_bytes / (ms * 1e-3) / 1e9,
                              'row_and_list_GBps': (row_bytes + list_bytes) / (ms * 1e-3) / 1e9}

# FlatGpuIndex on the same table: the index's own exhaustive search (its parent's search_batch over the same rows)
(fd, fi), flat_qps1 = timed(lambda qq: index.search_exhaustive(qq, limit=k), 1)
_, flat_qps2 = timed(lambda qq: index.search_exhaustive(qq, limit=k), 2)

links = index._gg.links[:N, 0].float()
print(json.dumps({'config': f'float HNSW (level 0, GPU-built): {N} x {D}-dim f32, L2, max_connection={a.max_connection}, '
                            f'ef_construction={a.ef_construction}, batch {B}, k={k}, {n_seeds} seeds',
                  'metric': 'queries/sec', 'unit': 'queries/s',
                  'value': res[f'ef_search_{a.ef_search[0]}']['queries_per_s_two_streams'],
                  'recall_at_10': res[f'ef_search_{a.ef_search[0]}']['recall_at_10'],
                  'build_s': build_s, 'build_rows_per_s': N / build_s, 'mean_links_per_node': float(links.mean().item()),
                  'flat_exact_queries_per_s_one_stream': flat_qps1, 'flat_exact_queries_per_s_two_streams': flat_qps2,
                  'steps': max(a.steps, 2), 'query_batches': 2, **res}))
