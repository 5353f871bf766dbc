#!/usr/bin/env python
"""Exact float32 search (FlatGpuIndex) against the torch formulation of the reference's FlatIndex
(annlite/core/index/flat_index.py:15-39: cdist + top_k) in the same process, alternating over rounds.  One JSON line.

    python scripts/bench_flat.py                       # 1M x 128, 1024 queries, k = 10, euclidean
    python scripts/bench_flat.py --rows 10000000
    python scripts/bench_flat.py --filter both         # the f32 and the split-bf16 filter, round by round: one JSON line each
    python scripts/bench_flat.py --filter both --offset 1000   # ... on data with a large common offset
    python scripts/bench_flat.py --rows both           # an f32-row index (default filter) and an f16-row index over the same data,
                                                       # round by round: one JSON line each (--rows 10000000 --rows both: at 10M)
    python scripts/bench_flat.py --rows all --data-scale 40    # ... and an int8-row index (dtype=np.int8) as the third: normal data
                                                       # scaled to the int8 range (3 sigma = 120 code steps)
    python scripts/bench_flat.py --rows f16i8 --data-scale 40  # the f16-row and the int8-row index alone (where the f32 twin does not fit)

Baseline: |x|^2 - 2 q x^T by torch.addmm over row chunks (no B x N matrix exists), torch.topk per chunk, one merge.
Filter time: the full-table filter launch (annlite_flat_filter with the bounds the search would hand it; for bf16x3
annlite_flat_filter_split, which also centres and splits the queries) between HIP events; its work is 2 B N D FLOP against the
157.3 TFLOP/s fp32 matrix roof -- the yardstick of both filters, whatever instruction they issue.
"""
import argparse
import json
import statistics
import sys
import os

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROOF_TFLOPS = 157.3
ROW_DTYPES = {'f32': ['f32'], 'f16': ['f16'], 'i8': ['i8'], 'both': ['f32', 'f16'], 'all': ['f32', 'f16', 'i8'], 'f16i8': ['f16', 'i8']}
ROW_FILTER = {'f32': 'f32', 'f16': 'f16x2', 'i8': 'i8x3'}


def row_dtypes(args):
    """``--rows both`` / ``all`` / ``f16i8`` / ``f32`` / ``f16`` / ``i8``: an f32-row FlatGpuIndex on its default filter -- the default
    path, untouched --, an f16-row one (``dtype=np.float16``) and an int8-row one (``dtype=np.int8``, default scale) over the same rows,
    alternating round by round in one process.  One JSON line per index."""
    import torch
    from annlite_amd import ops
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.enums import Metric

    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    N, D, B, k = args.rows, args.dim, args.batch, args.k
    metric = Metric.from_string(args.metric)
    l2 = metric == Metric.EUCLIDEAN
    kinds = ROW_DTYPES[args.row_dtype]
    np_dtype = {'f32': np.float32, 'f16': np.float16, 'i8': np.int8}
    index = {m: FlatGpuIndex(D, dtype=np_dtype[m], metric=metric, initial_size=N) for m in kinds}
    gen = torch.Generator(device=dev).manual_seed(0)
    step = 1 << 20
    truth_rows = []  # the UNROUNDED rows (as pre-processed), for the float64 truth; the f32 index holds them already
    for r0 in range(0, N, step):
        xb = torch.randn((min(step, N - r0), D), generator=gen, device=dev) * args.data_scale + args.offset
        for idx in index.values():
            idx.add_with_ids(xb, torch.arange(r0, r0 + xb.shape[0], device=dev))
        if 'f32' not in index:
            truth_rows.append(next(iter(index.values()))._pre(xb))
    q = torch.randn((B, D), generator=gen, device=dev) * args.data_scale + args.offset
    x_true = index['f32']._vectors[:N] if 'f32' in index else torch.cat(truth_rows)

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

    ms, answers, overflowed, last_counts = {m: [] for m in kinds}, {}, {}, {}
    for _ in range(args.rounds):
        for m in kinds:
            t, answers[m] = timed(lambda: index[m].search_batch(q, limit=k))
            ms[m].append(t)
            assert index[m].last_flat_filter == ROW_FILTER[m]
            overflowed[m] = index[m].last_overflowed
            last_counts[m] = ops.flat_list_counts(index[m]._ws, B).cpu().numpy()  # what the search's own last stage listed

    # the full-table filter alone, with the bound the search's last stage works with (see main())
    ratio = N / 4096.0
    n_stages = max(1, int(np.ceil(np.log(max(ratio, 1.0001)) / np.log(32.0) - 1e-9)))
    stride = max(1, int(ratio ** (1.0 / n_stages)))
    filter_ms = {}
    for m in kinds:
        idx = index[m]
        qq = idx._pre(q)
        n_sub = (N + stride - 1) // stride
        scale_kw = dict(int8_scale=idx.int8_scale_) if m == 'i8' else {}
        sub = FlatGpuIndex(D, dtype=np_dtype[m], metric=Metric.INNER_PRODUCT if metric == Metric.COSINE else metric, initial_size=n_sub,
                           **scale_kw)
        sub_rows = idx._vectors[:N:stride].float()
        if m == 'i8':
            sub_rows = sub_rows * idx.int8_scale_  # (the values the codes stand for: quantised again to the same codes)
        sub.add_with_ids(sub_rows.contiguous(), torch.arange(n_sub, device=dev))
        sd = sub.search_batch(qq, limit=k)[0][:, k - 1]
        bound = ((sd * sd) if l2 else sd).contiguous()
        del sub
        qn = ops.flat_row_norms(qq)

        def filter_once():
            if m == 'i8':
                return ops.flat_filter_i8(int(metric), qq, idx._vectors, idx._norms, bound, idx.int8_scale_, valid_bits=idx._valid, n_rows=N,
                                          workspace=idx._ws)
            if m == 'f16':
                return ops.flat_filter_f16(int(metric), qq, idx._vectors, idx._norms, bound, valid_bits=idx._valid, n_rows=N, workspace=idx._ws)
            return ops.flat_filter(int(metric), qq, idx._vectors, idx._norms, bound, valid_bits=idx._valid, n_rows=N, query_norms=qn)

        filter_once()
        f_ms = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            filter_once()
            e1.record()
            torch.cuda.synchronize()
            f_ms.append(e0.elapsed_time(e1))
        filter_ms[m] = statistics.median(f_ms)

    # recall@k of each index against float64 distances over the UNROUNDED rows: the price of the storage rounding
    nt = min(args.truth_queries, B)
    q64 = next(iter(index.values()))._pre(q)[:nt].double()
    best = None
    for r0 in range(0, N, 1 << 18):
        xc = x_true[r0:r0 + (1 << 18)].double()
        s = ((xc * xc).sum(1)[None, :] - 2.0 * q64 @ xc.T) if l2 else -(q64 @ xc.T)
        dd, ii = torch.topk(s, k, dim=1, largest=False)
        ii = ii + r0
        if best is not None:
            dd, ii = torch.cat([best[0], dd], 1), torch.cat([best[1], ii], 1)
            dd, p = torch.topk(dd, k, dim=1, largest=False)
            ii = torch.gather(ii, 1, p)
        best = (dd, ii)
    truth = best[1].cpu().numpy()
    flop = 2.0 * B * N * D
    for m in kinds:
        idx, med, f, count = index[m], statistics.median(ms[m]), filter_ms[m], last_counts[m]
        got = answers[m][1][:nt].cpu().numpy()
        held = sum(t.numel() * t.element_size() for t in (idx._vectors, idx._norms, idx._valid_bool))
        print(json.dumps({
            'bench': 'flat_rows', 'row_dtype': m, 'row_dtypes_in_this_run': kinds, 'flat_filter': idx.flat_filter, 'offset': args.offset,
            'data_scale': args.data_scale, 'int8_scale': idx.int8_scale_,
            'rows': N, 'dim': D, 'batch': B, 'k': k, 'metric': args.metric, 'rounds': args.rounds, 'steps': args.steps,
            'ms_per_batch': round(med, 4), 'qps': round(B / med * 1e3, 1), 'ms_rounds': [round(v, 4) for v in ms[m]],
            'filter_ms': round(f, 4), 'filter_tflops': round(flop / f / 1e9, 2),
            'filter_fraction_of_fp32_roof': round(flop / f / 1e9 / ROOF_TFLOPS, 4), 'filter_bound_rows_stride': stride,
            'candidates_mean': round(float(count.mean()), 1), 'candidates_max': int(count.max()),
            'overflowed_queries': int(overflowed[m]), 'hbm_bytes_held': int(held),
            'recall_at_k_vs_float64_unrounded_rows': float(np.mean([len(set(got[b]) & set(truth[b])) / k for b in range(nt)])),
            'truth_queries': nt, 'device': torch.cuda.get_device_name(0),
        }), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', action='append', default=[],
                    help="a number: rows of the table (default 1000000); f32 | f16 | i8 | both | all | f16i8: how the rows are stored -- "
                         "FlatGpuIndex(dtype=...), 'both': an f32-row and an f16-row index alternating, 'all': those and an int8-row one, "
                         "'f16i8': f16 and int8 alone (may be given twice: --rows 10000000 --rows all)")
    ap.add_argument('--dim', type=int, default=128)
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--metric', default='euclidean', choices=['euclidean', 'inner_product', 'cosine'])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=10, help='batches per round and path')
    ap.add_argument('--truth-queries', type=int, default=32)
    ap.add_argument('--chunk', type=int, default=65536, help='rows per chunk of the torch baseline')
    ap.add_argument('--filter', default='f32', choices=['f32', 'bf16x3', 'both'], help="FlatGpuIndex(flat_filter=...); 'both': alternating")
    ap.add_argument('--offset', type=float, default=0.0, help='added to every coordinate of rows and queries')
    ap.add_argument('--data-scale', type=float, default=1.0,
                    help='with --rows f32 | f16 | i8 | both | all | f16i8 only (an error otherwise): the standard deviation of every coordinate '
                         'of rows and queries (40: normal data in the int8 range)')
    args = ap.parse_args()
    given, args.rows, args.row_dtype = args.rows, 1_000_000, None
    for v in given:
        if v in ROW_DTYPES:
            args.row_dtype = v
        else:
            args.rows = int(v)
    if args.row_dtype is not None:
        assert args.filter == 'f32', '--rows f32 | f16 | i8 | both | all | f16i8 runs each index on its own default filter'
        return row_dtypes(args)
    assert args.data_scale == 1.0, '--data-scale belongs to the --rows f32 | f16 | i8 | both | all | f16i8 runs'

    import torch
    from annlite_amd import ops
    from annlite_amd.core.index.flat_gpu import FlatGpuIndex
    from annlite_amd.enums import Metric

    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    N, D, B, k = args.rows, args.dim, args.batch, args.k
    metric = Metric.from_string(args.metric)
    gen = torch.Generator(device=dev).manual_seed(0)
    modes = ['f32', 'bf16x3'] if args.filter == 'both' else [args.filter]
    # ONE index for both filters: built with the split filter's columns when that mode runs (centre = the first batch's mean), and
    # `flat_filter` switched between rounds -- the f32 path reads nothing the other mode added
    idx = FlatGpuIndex(D, metric=metric, initial_size=N, flat_filter=modes[-1])
    step = 1 << 20
    for r0 in range(0, N, step):  # (generated on the device: no 5 GB host array)
        n = min(step, N - r0)
        idx.add_with_ids(torch.randn((n, D), generator=gen, device=dev) + args.offset, torch.arange(r0, r0 + n, device=dev))
    q = torch.randn((B, D), generator=gen, device=dev) + args.offset
    x = idx._vectors[:N]
    l2 = metric == Metric.EUCLIDEAN

    def ours(mode):
        def run():
            idx.flat_filter = mode
            return idx.search_batch(q, limit=k)
        return run

    xn = (x * x).sum(1) if l2 else None

    def baseline():
        qq = idx._pre(q)
        best_d = best_i = None
        for r0 in range(0, N, args.chunk):
            xc = x[r0:r0 + args.chunk]
            if l2:
                s = torch.addmm(xn[r0:r0 + args.chunk][None, :], qq, xc.T, alpha=-2.0)  # |x|^2 - 2 q x^T  (+ |q|^2 after the top-k)
            else:
                s = -(qq @ xc.T)
            d, i = torch.topk(s, min(k, xc.shape[0]), dim=1, largest=False)
            i = i + r0
            if best_d is not None:
                d, i = torch.cat([best_d, d], 1), torch.cat([best_i, i], 1)
                d, p = torch.topk(d, k, dim=1, largest=False)
                i = torch.gather(i, 1, p)
            best_d, best_i = d, i
        if l2:
            best_d = torch.sqrt(torch.clamp(best_d + (qq * qq).sum(1)[:, None], min=0))
        else:
            best_d = 1.0 + best_d
        return best_d, best_i

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

    ms_ours, ms_base, answers, overflowed = {m: [] for m in modes}, [], {}, {}
    for _ in range(args.rounds):
        for m in modes:
            t, answers[m] = timed(ours(m))
            ms_ours[m].append(t)
            assert idx.last_flat_filter == m
            overflowed[m] = idx.last_overflowed
        t, (bd, bi) = timed(baseline)
        ms_base.append(t)
    for m in modes[1:]:  # the filters differ, the answer does not
        assert torch.equal(answers[m][0], answers[modes[0]][0]) and torch.equal(answers[m][1], answers[modes[0]][1])
    i = answers[modes[0]][1]

    # the full-table filter alone, with the bound the last stage works with: the k-th exact distance of the result itself is the
    # tightest the search can reach; the bound it really has (from 1/13 .. 1/32 of the table) lets a few hundred rows through
    qq = idx._pre(q)
    ratio = N / 4096.0
    n_stages = max(1, int(np.ceil(np.log(max(ratio, 1.0001)) / np.log(32.0) - 1e-9)))
    stride = max(1, int(ratio ** (1.0 / n_stages)))  # the last stage's bound comes from every stride-th row
    sub = FlatGpuIndex(D, metric=metric, initial_size=(N + stride - 1) // stride, flat_filter=modes[-1])
    sub.add_with_ids(x[::stride].contiguous(), torch.arange((N + stride - 1) // stride, device=dev))
    sd = sub.search_batch(q, limit=k)[0][:, k - 1]
    bound = ((sd * sd) if l2 else sd).contiguous()
    del sub
    qn = ops.flat_row_norms(qq)
    centred = idx._centre_dev is not None

    def filter_once(mode):
        if mode == 'f32':
            return ops.flat_filter(int(metric), qq, idx._vectors, idx._norms, bound, valid_bits=idx._valid, n_rows=N, query_norms=qn)[:2]
        return ops.flat_filter_split(int(metric), qq, idx._vectors, idx._cnorms if centred else idx._norms, bound,
                                     centre=idx._centre_dev, valid_bits=idx._valid, n_rows=N, workspace=idx._ws)[:2]

    filter_ms, counts = {}, {}
    for m in modes:
        filter_once(m)
        f_ms = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cand, count = filter_once(m)
            e1.record()
            torch.cuda.synchronize()
            f_ms.append(e0.elapsed_time(e1))
        filter_ms[m] = statistics.median(f_ms)
        counts[m] = count.cpu().numpy()

    # recall@k against float64 on a subset of the queries
    nt = min(args.truth_queries, B)
    q64 = qq[:nt].double()
    best = None
    for r0 in range(0, N, 1 << 18):
        xc = x[r0:r0 + (1 << 18)].double()
        s = ((xc * xc).sum(1)[None, :] - 2.0 * q64 @ xc.T) if l2 else -(q64 @ xc.T)
        dd, ii = torch.topk(s, k, dim=1, largest=False)
        ii = ii + r0
        if best is not None:
            dd, ii = torch.cat([best[0], dd], 1), torch.cat([best[1], ii], 1)
            dd, p = torch.topk(dd, k, dim=1, largest=False)
            ii = torch.gather(ii, 1, p)
        best = (dd, ii)
    truth = best[1].cpu().numpy()
    got, base_ids = i[:nt].cpu().numpy(), bi[:nt].cpu().numpy()
    recall = float(np.mean([len(set(got[b]) & set(truth[b])) / k for b in range(nt)]))
    recall_base = float(np.mean([len(set(base_ids[b]) & set(truth[b])) / k for b in range(nt)]))

    med_b = statistics.median(ms_base)
    flop = 2.0 * B * N * D
    for m in modes:
        med, f, count = statistics.median(ms_ours[m]), filter_ms[m], counts[m]
        print(json.dumps({
            'bench': 'flat_f32', 'flat_filter': m, 'filters_in_this_run': modes, 'offset': args.offset,
            'centred': bool(centred and m == 'bf16x3'), 'rows': N, 'dim': D, 'batch': B, 'k': k, 'metric': args.metric,
            'rounds': args.rounds, 'steps': args.steps,
            'ms_per_batch': round(med, 4), 'qps': round(B / med * 1e3, 1), 'ms_rounds': [round(v, 4) for v in ms_ours[m]],
            'baseline_torch_ms_per_batch': round(med_b, 4), 'baseline_torch_qps': round(B / med_b * 1e3, 1),
            'baseline_ms_rounds': [round(v, 4) for v in ms_base], 'speedup_vs_torch': round(med_b / med, 3),
            'filter_ms': round(f, 4), 'filter_tflops': round(flop / f / 1e9, 2),
            'filter_fraction_of_fp32_roof': round(flop / f / 1e9 / ROOF_TFLOPS, 4), 'roof_ms': round(flop / ROOF_TFLOPS / 1e9, 4),
            'filter_bound_rows_stride': stride, 'candidates_mean': round(float(count.mean()), 1), 'candidates_max': int(count.max()),
            'overflowed_queries': int(overflowed[m]), 'recall_at_k_vs_float64': recall, 'baseline_recall_at_k_vs_float64': recall_base,
            'truth_queries': nt, 'device': torch.cuda.get_device_name(0),
        }), flush=True)


if __name__ == '__main__':
    main()
