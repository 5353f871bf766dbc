#!/usr/bin/env python
"""The PCA projector on the GPU, one JSON line per measurement.

    python scripts/bench_projector.py                     # all three parts
    python scripts/bench_projector.py --parts a --rows-a 1024,1000000

(a) ``ops.affine_rows`` at n x 768 -> 128 against torch's ``(x - mean) @ M.T`` (rocBLAS) in the same process, alternating over rounds:
    the ratio, and the fraction of the roof -- the larger of FLOP / fp32 matrix peak and bytes / HBM peak (which of the two binds is
    reported).  (b) ``ops.pca_accumulate`` at 10240 x 768 (MAX_TRAINING_DATA_SIZE), with torch's f32 ``t.T @ t`` beside it.
(c) recall@10 of ``AnnLite(768, n_components=128, projector='gpu')`` (flat float index) against the exact un-projected top-10, on
    low-rank-plus-noise rows, and the queries per second of both facades (upload, projection, search and download included).
Times are HIP events around ``steps`` calls after a warm-up call; medians over ``rounds``.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROOF_TFLOPS = 157.3  # fp32 matrix peak
ROOF_TBPS = 8.0      # HBM3E peak


def _timed(torch, fn, steps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def part_a(args, torch, ops, dev):
    Din, Dout = args.dim, args.components
    gen = torch.Generator(device=dev).manual_seed(0)
    M = torch.randn((Dout, Din), generator=gen, device=dev) / Din ** 0.5
    mean = torch.randn((Din,), generator=gen, device=dev)
    for n in [int(v) for v in args.rows_a.split(',')]:
        x = torch.empty((n, Din), dtype=torch.float32, device=dev)
        for r0 in range(0, n, 1 << 20):
            x[r0:r0 + (1 << 20)] = torch.randn((min(1 << 20, n - r0), Din), generator=gen, device=dev) + mean
        out = torch.empty((n, Dout), dtype=torch.float32, device=dev)
        steps = max(args.steps, min(200, int(2e6 // max(n, 1))))  # (small batches: enough calls for a timed window)
        ours, base = [], []
        for _ in range(args.rounds):
            ours.append(_timed(torch, lambda: ops.affine_rows(x, M, sub=mean, out=out), steps))
            base.append(_timed(torch, lambda: torch.matmul(x - mean, M.T), steps))
        ref = torch.matmul((x[:4096] - mean).double(), M.T.double())
        err = float((out[:4096].double() - ref).abs().max())
        err_base = float((torch.matmul(x[:4096] - mean, M.T).double() - ref).abs().max())
        flop, nbytes = 2.0 * n * Din * Dout, 4.0 * (n * Din + n * Dout + Dout * Din)
        t_flop, t_mem = flop / ROOF_TFLOPS / 1e9, nbytes / ROOF_TBPS / 1e9  # ms
        med, med_b = statistics.median(ours), statistics.median(base)
        print(json.dumps({
            'bench': 'affine_rows', 'rows': n, 'din': Din, 'dout': Dout, 'rounds': args.rounds, 'steps': steps,
            'ms': round(med, 4), 'ms_rounds': [round(v, 4) for v in ours], 'torch_ms': round(med_b, 4),
            'torch_ms_rounds': [round(v, 4) for v in base], 'ratio_torch_over_ours': round(med_b / med, 3),
            'tflops': round(flop / med / 1e9, 2), 'tbytes_per_s': round(nbytes / med / 1e9, 3),
            'roof_ms': round(max(t_flop, t_mem), 4), 'roof_bound': 'fp32 mfma' if t_flop >= t_mem else 'hbm',
            'fraction_of_roof': round(max(t_flop, t_mem) / med, 4), 'max_abs_err_vs_f64': err, 'torch_max_abs_err_vs_f64': err_base,
            'device': torch.cuda.get_device_name(0)}), flush=True)
        del x, out


def part_b(args, torch, ops, dev):
    n, D = args.rows_b, args.dim
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((n, D), generator=gen, device=dev) + 3.0
    s = x[:1024].mean(dim=0).contiguous()
    sum64 = torch.zeros((D,), dtype=torch.float64, device=dev)
    gram64 = torch.zeros((D, D), dtype=torch.float64, device=dev)
    ws = ops.ScanWorkspace()
    steps = max(args.steps, 20)
    ours, base = [], []
    for _ in range(args.rounds):
        ours.append(_timed(torch, lambda: ops.pca_accumulate(x, s, sum64, gram64, ws), steps))

        def torch_gram():
            t = x - s
            return t.T @ t, t.sum(0)

        base.append(_timed(torch, torch_gram, steps))
    T = (D + 127) // 128
    flop = 2.0 * n * 128 * 128 * (T * (T + 1) // 2)  # the tiles that are computed (tj >= ti)
    med, med_b = statistics.median(ours), statistics.median(base)
    print(json.dumps({
        'bench': 'pca_accumulate', 'rows': n, 'dim': D, 'rounds': args.rounds, 'steps': steps, 'ms': round(med, 4),
        'ms_rounds': [round(v, 4) for v in ours], 'tflops_computed_tiles': round(flop / med / 1e9, 2),
        'fraction_of_fp32_roof': round(flop / med / 1e9 / ROOF_TFLOPS, 4), 'torch_f32_gram_ms': round(med_b, 4),
        'torch_ms_rounds': [round(v, 4) for v in base], 'ratio_torch_over_ours': round(med_b / med, 3),
        'device': torch.cuda.get_device_name(0)}), flush=True)


def part_c(args, torch, ops, dev):
    from annlite_amd import AnnLite
    from annlite_amd.index import Document, DocumentArray

    n, D, K, B, k = args.rows_c, args.dim, args.components, args.batch, 10
    rs = np.random.RandomState(2)
    basis = rs.randn(args.rank, D).astype(np.float32) / np.sqrt(args.rank)

    def make(m):
        return (rs.randn(m, args.rank).astype(np.float32) @ basis + args.noise * rs.randn(m, D).astype(np.float32)).astype(np.float32)

    x, q = make(n), make(B)
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, kw in (('projected', dict(n_components=K, projector='gpu')), ('unprojected', {})):
            ann = AnnLite(D, metric='euclidean', data_path=os.path.join(tmp, name), initial_size=n, **kw)
            t0 = time.perf_counter()
            ann.train(x[:10240])
            train_s = time.perf_counter() - t0
            for r0 in range(0, n, 65536):
                ann.index(DocumentArray([Document(id=str(r0 + i), embedding=v) for i, v in enumerate(x[r0:r0 + 65536])]))
            ann.search_numpy(q, limit=k)
            torch.cuda.synchronize()
            times = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    d, i = ann.search_numpy(q, limit=k)  # (returns numpy: the device work has finished)
                times.append((time.perf_counter() - t0) / args.steps)
            res[name] = dict(ids=np.stack(i), s=statistics.median(times), train_s=train_s)
    got, truth = res['projected']['ids'], res['unprojected']['ids']  # (the un-projected flat index is exact)
    recall = float(np.mean([len(set(got[b]) & set(truth[b])) / k for b in range(B)]))
    print(json.dumps({
        'bench': 'projected_flat_search', 'rows': n, 'dim': D, 'components': K, 'batch': B, 'k': k, 'rank': args.rank, 'noise': args.noise,
        'recall_at_10_vs_exact_unprojected': round(recall, 4),
        'projected_qps': round(B / res['projected']['s'], 1), 'unprojected_qps': round(B / res['unprojected']['s'], 1),
        'projected_ms_per_batch': round(res['projected']['s'] * 1e3, 3), 'unprojected_ms_per_batch': round(res['unprojected']['s'] * 1e3, 3),
        'projector_train_s_first_call': round(res['projected']['train_s'], 3), 'device': torch.cuda.get_device_name(0)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parts', default='abc')
    ap.add_argument('--dim', type=int, default=768)
    ap.add_argument('--components', type=int, default=128)
    ap.add_argument('--rows-a', default='1024,1000000,10000000')
    ap.add_argument('--rows-b', type=int, default=10240)
    ap.add_argument('--rows-c', type=int, default=200000)
    ap.add_argument('--batch', type=int, default=1024)
    ap.add_argument('--rank', type=int, default=64)
    ap.add_argument('--noise', type=float, default=0.05)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--steps', type=int, default=5)
    args = ap.parse_args()

    import torch
    from annlite_amd import ops

    torch.cuda.set_device(0)
    dev = torch.device('cuda', 0)
    for part, fn in (('a', part_a), ('b', part_b), ('c', part_c)):
        if part in args.parts:
            fn(args, torch, ops, dev)


if __name__ == '__main__':
    main()
