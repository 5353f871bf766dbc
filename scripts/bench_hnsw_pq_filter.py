#!/usr/bin/env python3
"""Filtered searches on the HNSW-over-PQ graph (HnswPQGpuIndex): for filters of several selectivities and the two
ranking modes (ADC sums, ``rerank=True``), queries/s and recall@10 of ``filter_search='graph'`` (the walk that lists admitted rows only)
and of ``filter_search='exact'`` (the parent's exhaustive masked scan: the default), the share of queries the graph path hands back to
the exact search, and -- once per mode -- the unfiltered walk.

    python scripts/bench_hnsw_pq_filter.py --rows 5000000        # tables on stderr, one JSON line on stdout

Filters: random subsets keeping the given fractions of the rows, and one correlated with the data (rows whose first coordinate lies
above a quantile).  Recall is against the exact filtered answer of the same ranking mode (``PQFlatGpuIndex``'s search on the same rows
and filter).  Each q/s is the median of ``--reps`` timed windows of at least ``--window`` seconds on one stream, the two paths
alternating, after a warm-up of both; a window ends in a device synchronise.  ``min_fraction`` (per mode) is the smallest measured
random fraction from which the graph path is BOTH faster than the exact one and within the margin of the unfiltered walk's recall, at
that and every larger measured fraction; the margin is tests/test_hnsw_pq_filter.py's: five standard deviations of a recall p over
batch x k answers, rounded up to a hundredth.  ``HnswPQGpuIndex.FILTER_WALK_MIN_FRACTION`` is set from the larger of the two modes'
(1.0 where no fraction qualifies).  Data and index: scripts/bench_hnsw.py's (M = 16 codes, the GPU-built graph), EUCLIDEAN.
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from annlite_amd import HnswPQGpuIndex, Metric, PQCodec  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--rows', type=int, default=5_000_000)
p.add_argument('--dim', type=int, default=128)
p.add_argument('--m', type=int, default=16)
p.add_argument('--batch', type=int, default=1024)
p.add_argument('--k', type=int, default=10)
p.add_argument('--ef-search', type=int, default=128)
p.add_argument('--ef-construction', type=int, default=200)
p.add_argument('--max-connection', type=int, default=16)
p.add_argument('--fractions', type=float, nargs='+', default=[0.5, 0.2, 0.1, 0.05, 0.02, 0.01])
p.add_argument('--correlated-quantile', type=float, default=0.84)
p.add_argument('--reps', type=int, default=3)
p.add_argument('--window', type=float, default=0.5)
a = p.parse_args()
dev = torch.device('cuda', 0)
torch.cuda.set_device(0)
N, D, M, B, k = a.rows, a.dim, a.m, a.batch, a.k
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


codec = PQCodec(dim=D, n_subvectors=M, n_clusters=256, metric=Metric.EUCLIDEAN, n_init=1)
codec.seed = 7
codec.deterministic = True
codec.fit(gen(0, 250_000)[:20480], iter=20)
index = HnswPQGpuIndex(dim=D, metric=Metric.EUCLIDEAN, pq_codec=codec, initial_size=N, rerank=True, ef_search=a.ef_search,
                       ef_construction=a.ef_construction, max_connection=a.max_connection, build='gpu')
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


gs = torch.Generator(device=dev)
gs.manual_seed(777)
u = torch.rand((N,), generator=gs, device=dev)
first = index._vectors[:N, 0]
filters = [(f'random {f:g}', torch.nonzero(u < f).reshape(-1)) for f in a.fractions]
filters.append((f'correlated (x[0] above its {a.correlated_quantile:g} quantile)',
                torch.nonzero(first > torch.quantile(first[:: max(1, N // 1_000_000)], a.correlated_quantile)).reshape(-1)))
ef = max(a.ef_search, k)
modes = {}
for mode, rerank in (('adc', False), ('rerank', True)):
    index.rerank = rerank
    truth = index.search_exhaustive(q, limit=k)[1]
    unf, unf_runs = measure({'walk': lambda qq: index.search_batch(qq, limit=k)})
    p_unf = recall(index.search_batch(q, limit=k)[1], truth)
    margin = math.ceil(5 * math.sqrt(p_unf * (1 - p_unf) / (B * k)) * 100 - 1e-9) / 100
    unfiltered = {'queries_per_s': unf['walk'], 'runs': unf_runs['walk'], 'recall_at_10': p_unf, 'margin': margin}
    rows_out = []
    for name, ids in filters:
        s = ids.numel() / N
        exact_d, exact_i = index.search_batch(q, limit=k, indices=ids, filter_search='exact')
        graph_d, graph_i = index.search_batch(q, limit=k, indices=ids, filter_search='graph')
        assert index.last_filter_path == 'graph'
        reanswered = index.last_filter_reanswered / B
        qps, runs = measure({'graph': lambda qq: index.search_batch(qq, limit=k, indices=ids, filter_search='graph'),
                             'exact': lambda qq: index.search_batch(qq, limit=k, indices=ids, filter_search='exact')})
        rows_out.append({'filter': name, 'fraction': s, 'ef_route': min(256, max(ef, -(-ef * N // max(ids.numel(), 1)))),
                         'graph_queries_per_s': qps['graph'], 'exact_queries_per_s': qps['exact'], 'graph_runs': runs['graph'],
                         'exact_runs': runs['exact'], 'graph_recall_at_10': recall(graph_i, exact_i), 'reanswered_share': reanswered})
    floor = p_unf - margin
    min_fraction = None
    for r, f in sorted(zip(rows_out[:len(a.fractions)], a.fractions), key=lambda t: -t[1]):  # from the densest filter down, while both hold
        if r['graph_queries_per_s'] > r['exact_queries_per_s'] and r['graph_recall_at_10'] >= floor:
            min_fraction = f
        else:
            break
    modes[mode] = {'unfiltered_walk': unfiltered, 'recall_floor': floor, 'min_fraction': min_fraction, 'filters': rows_out}
    print(f'[{mode}] unfiltered walk: {unfiltered["queries_per_s"] / 1e3:.0f} k q/s, recall@10 {p_unf:.4f} against the exhaustive search, '
          f'margin {margin:.2f}; min_fraction {min_fraction}', file=sys.stderr)
    print('| filter | share of rows | ef_route | graph q/s | exact q/s | graph recall@10 | re-answered |', file=sys.stderr)
    print('|---|---|---|---|---|---|---|', file=sys.stderr)
    for r in rows_out:
        print(f'| {r["filter"]} | {r["fraction"]:.4f} | {r["ef_route"]} | {r["graph_queries_per_s"] / 1e3:.0f} k | '
              f'{r["exact_queries_per_s"] / 1e3:.0f} k | {r["graph_recall_at_10"]:.4f} | {r["reanswered_share"]:.4f} |', file=sys.stderr)

fr = [m['min_fraction'] for m in modes.values()]
print(json.dumps({'config': f'HNSW-over-PQ filtered search: {N} x {D}-dim, M={M}, L2, max_connection={a.max_connection}, '
                            f'ef_construction={a.ef_construction}, ef_search={a.ef_search}, batch {B}, k={k}, one stream',
                  'metric': 'queries/sec', 'unit': 'queries/s', 'value': modes['adc']['filters'][0]['graph_queries_per_s'],
                  'reps': a.reps, 'window_s': a.window, 'min_fraction': 1.0 if None in fr else max(fr), 'modes': modes}))
