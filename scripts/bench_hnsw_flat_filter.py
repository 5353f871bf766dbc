#!/usr/bin/env python3
"""Filtered searches on the float HNSW graph (HnswFlatGpuIndex): for filters of several selectivities, queries/s
and recall@10 of ``filter_search='graph'`` (the walk that lists admitted rows only) and of ``filter_search='exact'`` (the parent's exact
filtered search: the default), the share of queries the graph path hands back to the exact search, and -- once -- the unfiltered walk.

    python scripts/bench_hnsw_flat_filter.py --rows 1000000        # a table on stderr, one JSON line on stdout

Filters: random subsets keeping the given fractions of the rows, and one correlated with the data (rows whose first coordinate lies
above a quantile).  Recall is against the exact filtered answer (``FlatGpuIndex``'s search on the same rows and filter).  Each q/s is
the median of ``--reps`` timed windows of at least ``--window`` seconds, the two paths alternating, after a warm-up of both; a window
ends in a device synchronise.  ``min_fraction`` is the smallest measured random fraction from which the graph path is BOTH faster than
the exact one and within 0.03 of the unfiltered walk's recall, at that and every larger measured fraction: what
``HnswFlatGpuIndex.FILTER_WALK_MIN_FRACTION`` is set from.  Data: scripts/bench_hnsw_flat.py's generator, EUCLIDEAN.
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
from annlite_amd import HnswFlatGpuIndex, Metric  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--rows', type=int, default=1_000_000)
p.add_argument('--dim', type=int, default=128)
p.add_argument('--batch', type=int, default=1024)
p.add_argument('--k', type=int, default=10)
p.add_argument('--ef-search', type=int, default=64)
p.add_argument('--ef-construction', type=int, default=200)
p.add_argument('--max-connection', type=int, default=16)
p.add_argument('--fractions', type=float, nargs='+', default=[0.5, 0.2, 0.1, 0.05, 0.02, 0.01])
p.add_argument('--correlated-quantile', type=float, default=0.84)
p.add_argument('--reps', type=int, default=3)
p.add_argument('--window', type=float, default=0.5)
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


index = HnswFlatGpuIndex(D, metric=Metric.EUCLIDEAN, initial_size=N, ef_search=a.ef_search, ef_construction=a.ef_construction,
                         max_connection=a.max_connection)
for c in range((N + CH - 1) // CH):
    rows = min(CH, N - c * CH)
    index.add_with_ids(gen(c, rows), torch.arange(c * CH, c * CH + rows, device=dev, dtype=torch.int64))
torch.cuda.synchronize()
q_rot = [queries(4321), queries(4321 + 7919)]  # the timed steps rotate through two query batches (recall is the first batch's)
q = q_rot[0]


def recall(ids, truth):
    ids, truth = ids.cpu().numpy(), truth.cpu().numpy()
    return float(np.mean([len(set(ids[b]) & set(truth[b])) / k for b in range(B)]))


def window(fn):
    """q/s of one timed window: batches until ``--window`` seconds have passed (at least 8), closed by a synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while n < 8 or time.perf_counter() - t0 < a.window:
        fn(q_rot[n % 2])
        n += 1
        if n % 8 == 0:
            torch.cuda.synchronize()  # (the queue stays short: the clock is read against finished work)
    torch.cuda.synchronize()
    return B * n / (time.perf_counter() - t0)


def measure(fns):
    """{name: median q/s} of the callables, alternating, ``--reps`` windows each after a warm-up of every one"""
    for fn in fns.values():
        for j in range(4):
            fn(q_rot[j % 2])
    torch.cuda.synchronize()
    runs = {name: [] for name in fns}
    for _ in range(a.reps):
        for name, fn in fns.items():
            runs[name].append(window(fn))
    return {name: float(np.median(v)) for name, v in runs.items()}, runs


truth = index.search_exhaustive(q, limit=k)[1]
unf, unf_runs = measure({'walk': lambda qq: index.search_batch(qq, limit=k)})
unfiltered = {'queries_per_s': unf['walk'], 'runs': unf_runs['walk'], 'recall_at_10': recall(index.search_batch(q, limit=k)[1], truth)}

gs = torch.Generator(device=dev)
gs.manual_seed(777)
u = torch.rand((N,), generator=gs, device=dev)
first = index._vectors[:N, 0]
filters = [(f'random {f:g}', torch.nonzero(u < f).reshape(-1)) for f in a.fractions]
filters.append((f'correlated (x[0] above its {a.correlated_quantile:g} quantile)',
                torch.nonzero(first > torch.quantile(first[:: max(1, N // 1_000_000)], a.correlated_quantile)).reshape(-1)))

rows_out = []
for name, ids in filters:
    s = ids.numel() / N
    exact_d, exact_i = index.search_batch(q, limit=k, indices=ids, filter_search='exact')
    graph_d, graph_i = index.search_batch(q, limit=k, indices=ids, filter_search='graph')
    assert index.last_filter_path == 'graph'
    reanswered = index.last_filter_reanswered / B
    qps, runs = measure({'graph': lambda qq: index.search_batch(qq, limit=k, indices=ids, filter_search='graph'),
                         'exact': lambda qq: index.search_batch(qq, limit=k, indices=ids, filter_search='exact')})
    ef = max(a.ef_search, k)
    rows_out.append({'filter': name, 'fraction': s, 'ef_route': min(256, max(ef, -(-ef * N // max(ids.numel(), 1)))),
                     'graph_queries_per_s': qps['graph'], 'exact_queries_per_s': qps['exact'], 'graph_runs': runs['graph'],
                     'exact_runs': runs['exact'], 'graph_recall_at_10': recall(graph_i, exact_i),
                     'exact_recall_at_10': recall(exact_i, exact_i), 'reanswered_share': reanswered})

floor = unfiltered['recall_at_10'] - 0.03
min_fraction = None
for r, f in sorted(zip(rows_out[:len(a.fractions)], a.fractions), key=lambda t: -t[1]):  # from the densest filter down, while both hold
    if r['graph_queries_per_s'] > r['exact_queries_per_s'] and r['graph_recall_at_10'] >= floor:
        min_fraction = f
    else:
        break

print(f'unfiltered walk: {unfiltered["queries_per_s"] / 1e3:.0f} k q/s, recall@10 {unfiltered["recall_at_10"]:.4f}', file=sys.stderr)
print('| filter | share of rows | ef_route | graph q/s | exact q/s | graph recall@10 | exact recall@10 | re-answered |', file=sys.stderr)
print('|---|---|---|---|---|---|---|---|', file=sys.stderr)
for r in rows_out:
    print(f'| {r["filter"]} | {r["fraction"]:.4f} | {r["ef_route"]} | {r["graph_queries_per_s"] / 1e3:.0f} k | '
          f'{r["exact_queries_per_s"] / 1e3:.0f} k | {r["graph_recall_at_10"]:.4f} | {r["exact_recall_at_10"]:.4f} | '
          f'{r["reanswered_share"]:.4f} |', file=sys.stderr)
print(json.dumps({'config': f'float HNSW filtered search: {N} x {D}-dim f32, L2, max_connection={a.max_connection}, '
                            f'ef_construction={a.ef_construction}, ef_search={a.ef_search}, batch {B}, k={k}',
                  'metric': 'queries/sec', 'unit': 'queries/s', 'value': rows_out[0]['graph_queries_per_s'],
                  'reps': a.reps, 'window_s': a.window, 'unfiltered_walk': unfiltered, 'recall_floor': floor,
                  'min_fraction': min_fraction, 'filters': rows_out}))
