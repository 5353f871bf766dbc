#!/usr/bin/env python
"""Cells over float vectors (IvfFlatGpuIndex) against the exhaustive exact search (FlatGpuIndex.search_batch)
over the SAME rows, in the same process, alternating over rounds.  One JSON line per run, appended to
profiles/ivf_flat/bench_ivf_flat.jsonl.

    python scripts/bench_ivf_flat.py                                   # 1M x 128 i.i.d. normal, 1024 queries, k = 10, 16 of 256 cells
    python scripts/bench_ivf_flat.py --rows 10000000 --data lowrank    # the low-rank data of tests/test_ivf.py::_data
    python scripts/bench_ivf_flat.py --filter both                     # cell_filter='f32' against 'bf16x3' 
    python scripts/bench_ivf_flat.py --filter both --offset 1000       # ... on data with a common offset

--filter both: two indexes over the same rows and the same codebook, one per cell filter; the paths alternate round by round in this
process.  The top-level `pruned_*` / `list_*` / `overflowed_queries` keys describe the first path (`filter`); `paths` holds, per filter
name, the time per batch, the filter kernel's time, the list mean / max and the overflow count.

Recall: against the exhaustive search's answer, which is exact.  Filter time: the launches of the path's filter kernel
(ivf_flat_filter_kernel / ivf_flat_split_filter_kernel) in one search, from the profiler's kernel records (null where the profiler
records no kernels); `pruned_search_kernels` lists every kernel of that search as (launches, ms).
"""
FILTER_KERNEL = {'f32': 'ivf_flat_filter_kernel', 'bf16x3': 'ivf_flat_split_filter_kernel'}
import argparse
import json
import os
import re
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=1_000_000)
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--cells', type=int, default=256)
    ap.add_argument('--probe', type=int, default=16)
    ap.add_argument('--data', default='normal', choices=['normal', 'lowrank'])
    ap.add_argument('--filter', default='f32', choices=['f32', 'bf16x3', 'both'], help='cell_filter of the pruned path(s)')
    ap.add_argument('--offset', type=float, default=0.0, help='added to rows, training rows and queries')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5, help='batches per round and path')
    ap.add_argument('--train-rows', type=int, default=65536)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ivf_flat', 'bench_ivf_flat.jsonl'))
    args = ap.parse_args()

    import torch
    from annlite_amd import ops
    from annlite_amd.core.codec.vq import VQCodec
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex
    from annlite_amd.enums import Metric

    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    N, D, B, k, C, P = args.rows, args.dim, args.batch, args.k, args.cells, args.probe
    metric = Metric.EUCLIDEAN
    gen = torch.Generator(device=dev).manual_seed(0)
    A = torch.randn((8, D), generator=gen, device=dev)

    def draw(n):  # (generated on the device: no 5 GB host array)
        if args.data == 'normal':
            x = torch.randn((n, D), generator=gen, device=dev)
        else:
            x = torch.randn((n, 8), generator=gen, device=dev) @ A + 0.1 * torch.randn((n, D), generator=gen, device=dev)
        return x + args.offset if args.offset else x

    step = 1 << 20
    first = draw(min(step, N))
    vq = VQCodec(C, metric=metric, iter=10, n_init=1)
    vq.seed = 1
    vq.fit(first[:args.train_rows].contiguous())
    filters = ['f32', 'bf16x3'] if args.filter == 'both' else [args.filter]
    paths = {f: IvfFlatGpuIndex(D, vq_codec=vq, n_probe=P, metric=metric, initial_size=N, cell_filter=f) for f in filters}
    for r0 in range(0, N, step):
        n = min(step, N - r0)
        chunk = first if r0 == 0 else draw(n)
        for p in paths.values():
            p.add_with_ids(chunk, torch.arange(r0, r0 + n, device=dev))
    del first, chunk
    idx = paths[filters[0]]
    q = draw(B)

    def exhaustive():
        return FlatGpuIndex.search_batch(idx, q, limit=k)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps, out

    ms_p, ms_e, answers = {f: [] for f in filters}, [], {}
    for _ in range(args.rounds):
        t, (de, ie) = timed(exhaustive)
        ms_e.append(t)
        over_e = idx.last_overflowed
        for f in filters:
            t, answers[f] = timed(lambda: paths[f].search_batch(q, limit=k))
            ms_p[f].append(t)
    for f in filters[1:]:  # (the filters differ in what they list, never in the answer)
        assert torch.equal(answers[f][1], answers[filters[0]][1]) and torch.equal(answers[f][0], answers[filters[0]][0]), f
    dp, ip = answers[filters[0]]
    sizes = (idx._cell_rows[:, 1] - idx._cell_rows[:, 0]).cpu().numpy()
    max_probed = int(idx._sizes_cum[P - 1])

    def one_search(p, f):
        """(filter kernel ms, {kernel: (launches, ms)}) of one search of path p, from the profiler's kernel records"""
        filter_ms, kernels = None, {}
        try:
            from torch.profiler import ProfilerActivity, profile

            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                p.search_batch(q, limit=k)
                torch.cuda.synchronize()
            dev_us = lambda e: e.device_time_total if hasattr(e, 'device_time_total') else e.cuda_time_total
            us = [dev_us(e) for e in prof.key_averages() if FILTER_KERNEL[f] in e.key]
            filter_ms = round(sum(us) / 1e3, 4) if us else None
            for e in prof.key_averages():  # every kernel of the one search: (launches, ms), by the name in front of the template arguments
                if dev_us(e) > 0:
                    name = e.key.split('(')[0].split('<')[0].split('::')[-1]
                    m = re.match(r'_ZN7annlite(\d+)', name)  # (a name the profiler's demangler left alone: __bf16 arguments)
                    if m:
                        name = name[m.end():m.end() + int(m.group(1))]
                    n, ms = kernels.get(name, (0, 0.0))
                    kernels[name] = (n + e.count, round(ms + dev_us(e) / 1e3, 4))
        except Exception as ex:  # (the measurement is optional; the rest of the line stands)
            filter_ms = None
            print('profiler: %r' % (ex,), file=sys.stderr)
        return filter_ms, kernels

    report = {}
    for f in filters:
        p = paths[f]
        p.search_batch(q, limit=k)
        count = ops.flat_list_counts(p._ws, B).cpu().numpy()
        filter_ms, kernels = one_search(p, f)
        med = statistics.median(ms_p[f])
        report[f] = {'ms_per_batch': round(med, 4), 'qps': round(B / med * 1e3, 1), 'ms_rounds': [round(v, 4) for v in ms_p[f]],
                     'filter_kernel': FILTER_KERNEL[f], 'filter_kernel_ms': filter_ms, 'kernels': kernels,
                     'list_mean': round(float(count.mean()), 1), 'list_max': int(count.max()), 'overflowed_queries': int(p.last_overflowed),
                     'last_cell_filter': p.last_cell_filter}
    main_path = report[filters[0]]
    ms_p, filter_ms, kernels = ms_p[filters[0]], main_path['filter_kernel_ms'], main_path['kernels']

    ie_np, ip_np = ie.cpu().numpy(), ip.cpu().numpy()
    recall = float(np.mean([len(set(ip_np[b]) & set(ie_np[b])) / k for b in range(B)]))
    med_p, med_e = statistics.median(ms_p), statistics.median(ms_e)
    line = json.dumps({
        'bench': 'ivf_flat_f32', 'filter': filters[0], 'offset': args.offset, 'rows': N, 'dim': D, 'batch': B, 'k': k, 'metric': 'euclidean', 'data': args.data, 'n_cells': C, 'n_probe': P,
        'rounds': args.rounds, 'steps': args.steps,
        'pruned_ms_per_batch': round(med_p, 4), 'pruned_qps': round(B / med_p * 1e3, 1), 'pruned_ms_rounds': [round(v, 4) for v in ms_p],
        'exhaustive_ms_per_batch': round(med_e, 4), 'exhaustive_qps': round(B / med_e * 1e3, 1),
        'exhaustive_ms_rounds': [round(v, 4) for v in ms_e], 'speedup_vs_exhaustive': round(med_e / med_p, 3),
        'ivf_flat_filter_kernel_ms': filter_ms, 'pruned_search_kernels': kernels,
        'paths': {f: {key: v for key, v in r.items() if key != 'kernels' or f != filters[0]} for f, r in report.items()}, 'strides': ops.ivf_flat_stages(max_probed), 'max_probed_rows': max_probed,
        'cell_rows_max': int(sizes.max()), 'cell_rows_mean': round(float(sizes.mean()), 1), 'cell_rows_min': int(sizes.min()),
        'list_mean': main_path['list_mean'], 'list_max': main_path['list_max'], 'overflowed_queries': main_path['overflowed_queries'],
        'exhaustive_overflowed_queries': int(over_e), 'recall_at_k_vs_exhaustive': round(recall, 4),
        'device': torch.cuda.get_device_name(0),
    })
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
