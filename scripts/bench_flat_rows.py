#!/usr/bin/env python3
"""Filtered exact float search ("selected rows"): ``filter_route='rows'`` against ``'mask'``, and what
``annlite_bitmap_rows`` costs alone.

    python scripts/bench_flat_rows.py                      # tables on stderr, one JSON line on stdout

Search (``--rows`` x ``--dim``, default 1M x 128; ``k = 10``; batches of ``--batches``, default 1024 and 64; row types f32, f16, int8):
one ``FlatGpuIndex`` per row type, EUCLIDEAN, i.i.d. normal rows made on the device.  Selections: random ones keeping ``--shares`` of
the rows and one clustered -- the first 5 % of the offsets --, each handed over as a ``RowMask`` (what a filter evaluated on the device
gives the index).  Per case the two routes ALTERNATE in one process: a warm-up call each, then two timings each, a timing being the host
clock around ``--calls`` whole ``search_batch`` calls that ends in a device synchronise -- so the ``'rows'`` figure holds the compaction
and the host read of the selection's size.  ``spread``: the larger of the two routes' differences between their two timings; ``'rows'``
counts as faster where the slower of its timings beats the faster of the mask's by more than that.  The answers of the two routes are
compared on every case.  ``--big-rows`` (default 10M; 0: skip): one f32 case at 1 %.

Kernel: ``annlite_bitmap_rows`` alone, one pair of device events around ``--launches`` back-to-back calls after a warm-up, the median
of ``--reps`` windows; ``bytes``: N / 8 read and 4 n written, from the shapes; ``share``: bytes over that time against the HBM peak of
8.0 TB/s.
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
from annlite_amd import ops  # noqa: E402
from annlite_amd.columns import RowMask  # noqa: E402
from annlite_amd.core.index.flat_gpu import FlatGpuIndex  # noqa: E402
from annlite_amd.enums import Metric  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s: the part's specification

p = argparse.ArgumentParser()
p.add_argument('--rows', type=int, default=1_000_000)
p.add_argument('--big-rows', type=int, default=10_000_000)
p.add_argument('--dim', type=int, default=128)
p.add_argument('--batches', type=int, nargs='+', default=[1024, 64])
p.add_argument('--shares', type=float, nargs='+', default=[0.5, 0.2, 0.1, 0.05, 0.01, 0.001])
p.add_argument('--types', nargs='+', default=['f32', 'f16', 'i8'])
p.add_argument('--calls', type=int, default=10)
p.add_argument('--launches', type=int, default=200)
p.add_argument('--reps', type=int, default=3)
a = p.parse_args()
torch.cuda.set_device(0)
dev = torch.device('cuda', 0)
K = 10
TYPES = {'f32': dict(), 'f16': dict(dtype=np.float16), 'i8': dict(dtype=np.int8)}


def pack(flags):
    """bool [n] on the device -> i32 words"""
    n = flags.numel()
    padded = torch.zeros(((n + 31) // 32 * 32,), dtype=torch.bool, device=dev)
    padded[:n] = flags
    return FlatGpuIndex._pack_bits(padded)


def make_index(kind, n):
    idx = FlatGpuIndex(a.dim, metric=Metric.EUCLIDEAN, initial_size=n, **TYPES[kind])
    g = torch.Generator(device=dev).manual_seed(1)
    for lo in range(0, n, 1_000_000):
        hi = min(n, lo + 1_000_000)
        x = torch.randn((hi - lo, a.dim), generator=g, device=dev)
        idx.add_with_ids(x * 20 if kind == 'i8' else x, torch.arange(lo, hi, device=dev))  # (int8: codes of a few dozen steps)
    return idx


def selections(n, shares):
    g = torch.Generator(device=dev).manual_seed(2)
    out = []
    for s in shares:
        flags = torch.rand((n,), generator=g, device=dev) < s
        out.append(('random %g' % s, flags))
    head = torch.zeros((n,), dtype=torch.bool, device=dev)
    head[: n // 20] = True
    out.append(('first 0.05', head))
    return [(name, RowMask(pack(f), f.sum().reshape(1), n), int(f.sum().item())) for name, f in out]


def timing(idx, q, mask, route):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.calls):
        ans = idx.search_batch(q, limit=K, indices=mask, filter_route=route)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / a.calls, ans


def search_cases(kind, n, batches, sels, result):
    idx = make_index(kind, n)
    g = torch.Generator(device=dev).manual_seed(3)
    for B in batches:
        q = torch.randn((B, a.dim), generator=g, device=dev) * (20 if kind == 'i8' else 1)
        for name, mask, n_sel in sels:
            t = {'mask': [], 'rows': []}
            ans = {}
            for rep in range(3):  # (a warm-up, then the two timings)
                for route in ('mask', 'rows'):
                    dt, ans[route] = timing(idx, q, mask, route)
                    assert idx.last_filter_route == route
                    if rep:
                        t[route].append(dt)
            same = torch.equal(ans['mask'][1], ans['rows'][1]) and torch.equal(ans['mask'][0].view(torch.int32), ans['rows'][0].view(torch.int32))
            spread = max(abs(t['mask'][0] - t['mask'][1]), abs(t['rows'][0] - t['rows'][1]))
            row = dict(type=kind, rows=n, dim=a.dim, batch=B, selection=name, share=n_sel / n, n_sel=n_sel, mask_ms=[v * 1e3 for v in t['mask']],
                       rows_ms=[v * 1e3 for v in t['rows']], spread_ms=spread * 1e3, rows_faster=bool(max(t['rows']) + spread < min(t['mask'])),
                       same_answer=bool(same), mask_qps=B / min(t['mask']), rows_qps=B / min(t['rows']))
            result['search'].append(row)
            print('%4s %9d %5d %-12s %9d  mask %8.3f %8.3f  rows %8.3f %8.3f  spread %6.3f  %5.2fx %s %s' % (
                kind, n, B, name, n_sel, *row['mask_ms'], *row['rows_ms'], row['spread_ms'], min(t['mask']) / min(t['rows']),
                'rows' if row['rows_faster'] else '-', '' if same else 'ANSWERS DIFFER'), file=sys.stderr)
    del idx
    torch.cuda.empty_cache()


def kernel_cases(n, result):
    g = torch.Generator(device=dev).manual_seed(4)
    out = torch.empty((n,), dtype=torch.int32, device=dev)
    ws = ops.ScanWorkspace()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for share in (0.5, 0.1, 0.01):
        flags = torch.rand((n,), generator=g, device=dev) < share
        words, n_sel = pack(flags), int(flags.sum().item())
        for _ in range(20):
            ops.bitmap_rows(words, n_rows=n, out=out, workspace=ws, sync=False)
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            s.record()
            for _ in range(a.launches):
                ops.bitmap_rows(words, n_rows=n, out=out, workspace=ws, sync=False)
            e.record()
            torch.cuda.synchronize()
            times.append(s.elapsed_time(e) / a.launches * 1e-3)
        sec = float(np.median(times))
        nbytes = n // 8 + 4 * n_sel
        assert int(ops.bitmap_rows(words, n_rows=n, out=out, workspace=ws)[1]) == n_sel
        row = dict(rows=n, share=share, n_sel=n_sel, us=sec * 1e6, bytes=nbytes, share_of_hbm_peak=nbytes / sec / HBM_PEAK)
        result['kernel'].append(row)
        print('bitmap_rows %9d rows  %5.3f selected  %8.1f us  %8.2f MB  %6.4f of the HBM peak' % (n, share, sec * 1e6, nbytes / 1e6,
                                                                                               row['share_of_hbm_peak']), file=sys.stderr)


result = {'search': [], 'kernel': []}
print('type      rows batch selection        n_sel  ms per call, two timings each', file=sys.stderr)
sels = selections(a.rows, a.shares)
for kind in a.types:
    search_cases(kind, a.rows, a.batches, sels, result)
del sels
if a.big_rows:
    search_cases('f32', a.big_rows, a.batches[:1], selections(a.big_rows, [0.01])[:1], result)
for n in [a.rows] + ([a.big_rows] if a.big_rows else []):
    kernel_cases(n, result)
# the largest measured share at which 'rows' is faster for every row type and batch size
by_share = {}
for r in result['search']:
    if r['rows'] == a.rows and r['selection'].startswith('random'):
        by_share.setdefault(r['selection'], []).append(r['rows_faster'])
winners = [float(name.split()[1]) for name, v in by_share.items() if all(v)]
result['rows_max_fraction'] = max(winners) if winners else None
result['all_answers_same'] = all(r['same_answer'] for r in result['search'])
print('rows is faster for every row type and batch size up to a share of', result['rows_max_fraction'], file=sys.stderr)
print(json.dumps(result))
