#!/usr/bin/env python3
"""Exact float search with ``limit > 64`` ("limit above 64"): ``large_k='wide'`` against ``'host'``.

    python scripts/bench_flat_wide.py                      # tables on stderr, one JSON line on stdout

Table search (``--rows`` x ``--dim``, default 1M x 128; ``--limits``, default 100 and 1000; batches of ``--batches``, default 1024 and
64; row types f32, f16, int8): one ``FlatGpuIndex`` per row type, EUCLIDEAN, i.i.d. normal rows made on the device.  Pruned cell search:
an ``IvfFlatGpuIndex`` over the same f32 rows, ``--cells`` cells (default 256; i.i.d. normal centroids) of which ``--probe``
(default 16) are probed, the first limit.  Per case the two values ALTERNATE in one process: a warm-up call each, then two timings each,
a timing being the host clock around whole ``search_batch`` calls (as many as fit ``--seconds``, at most ``--calls``) that ends in a
device synchronise.  ``spread``: the larger of the two differences between a value's two timings; ``'wide'`` counts as not slower where
its slower timing does not exceed the faster of the host's by more than that.  The answers are compared on every case.

Device: ``annlite_flat_search_topk_wide`` alone (``ops``: no index, no pre-processing) between a pair of device events, the median of
``--reps`` windows, and the one filter stage inside it alone (``ops.flat_filter*`` against the bound +inf costs what any bound costs:
the contraction does not depend on it) -- what remains is the three launches of the wide kernel (sample, lists, overflow route).
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
from annlite_amd.core.codec.vq import VQCodec  # noqa: E402
from annlite_amd.core.index.flat_gpu import FlatGpuIndex  # noqa: E402
from annlite_amd.core.index.ivf_flat_gpu import IvfFlatGpuIndex  # noqa: E402
from annlite_amd.enums import Metric  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--rows', type=int, default=1_000_000)
p.add_argument('--dim', type=int, default=128)
p.add_argument('--batches', type=int, nargs='+', default=[1024, 64])
p.add_argument('--limits', type=int, nargs='+', default=[100, 1000])
p.add_argument('--types', nargs='+', default=['f32', 'f16', 'i8'])
p.add_argument('--cells', type=int, default=256)
p.add_argument('--probe', type=int, default=16)
p.add_argument('--calls', type=int, default=10)
p.add_argument('--seconds', type=float, default=1.0)
p.add_argument('--reps', type=int, default=3)
a = p.parse_args()
torch.cuda.set_device(0)
dev = torch.device('cuda', 0)
TYPES = {'f32': dict(), 'f16': dict(dtype=np.float16), 'i8': dict(dtype=np.int8)}


def fill(idx, kind):
    g = torch.Generator(device=dev).manual_seed(1)
    for lo in range(0, a.rows, 1_000_000):
        hi = min(a.rows, lo + 1_000_000)
        x = torch.randn((hi - lo, a.dim), generator=g, device=dev)
        idx.add_with_ids(x * 20 if kind == 'i8' else x, torch.arange(lo, hi, device=dev))  # (int8: codes of a few dozen steps)
    return idx


def timing(idx, q, k, value, calls, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        ans = idx.search_batch(q, limit=k, large_k=value, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls, ans


def compare(idx, what, kind, q, k, result, **kw):
    t, ans, calls = {'host': [], 'wide': []}, {}, {'host': 1, 'wide': 1}
    for rep in range(3):  # (a warm-up, which also sizes the timings, then the two timings)
        for value in ('host', 'wide'):
            dt, ans[value] = timing(idx, q, k, value, calls[value], **kw)
            assert idx.last_large_k == value
            if rep:
                t[value].append(dt)
            else:
                calls[value] = int(min(a.calls, max(1, a.seconds / dt)))
    same = torch.equal(ans['host'][1], ans['wide'][1]) and torch.equal(ans['host'][0].view(torch.int32), ans['wide'][0].view(torch.int32))
    spread = max(abs(t['host'][0] - t['host'][1]), abs(t['wide'][0] - t['wide'][1]))
    row = dict(search=what, type=kind, rows=a.rows, dim=a.dim, batch=q.shape[0], limit=k, host_ms=[v * 1e3 for v in t['host']],
               wide_ms=[v * 1e3 for v in t['wide']], spread_ms=spread * 1e3, wide_not_slower=bool(max(t['wide']) <= min(t['host']) + spread),
               same_answer=bool(same), overflowed=int(idx.last_overflowed))
    result['search'].append(row)
    print('%-5s %4s %5d %5d  host %9.3f %9.3f  wide %9.3f %9.3f  spread %7.3f  %6.2fx %s %s' % (
        what, kind, q.shape[0], k, *row['host_ms'], *row['wide_ms'], row['spread_ms'], min(t['host']) / min(t['wide']),
        'ok' if row['wide_not_slower'] else 'WIDE SLOWER', '' if same else 'ANSWERS DIFFER'), file=sys.stderr)


def events(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    times = []
    for _ in range(a.reps):
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return float(np.median(times))


def device_cases(idx, kind, q, k, result):
    ws = ops.ScanWorkspace()
    scale = idx.int8_scale_ or 1.0
    whole = events(lambda: ops.flat_search_topk_wide(idx._kind.tag, 1, q, idx._vectors, idx._norms, k, valid_bits=idx._valid, n_rows=a.rows,
                                                     scale=scale, sqrt=True, workspace=ws))
    inf = torch.full((q.shape[0],), float('inf'), device=dev)
    stage = events(lambda: idx._kind.stage(1, q, idx._vectors, idx._norms, inf, valid_bits=idx._valid, n_rows=a.rows))
    result['device'].append(dict(type=kind, batch=q.shape[0], limit=k, call_ms=whole, filter_stage_ms=stage, wide_kernels_ms=whole - stage))
    print('device %4s %5d %5d  call %9.3f ms  filter stage %8.3f ms  wide kernels %9.3f ms' % (kind, q.shape[0], k, whole, stage, whole - stage),
          file=sys.stderr)


result = {'search': [], 'device': []}
print('search type batch limit  ms per call, two timings each', file=sys.stderr)
g = torch.Generator(device=dev).manual_seed(3)
queries = {B: torch.randn((B, a.dim), generator=g, device=dev) for B in a.batches}
for kind in a.types:
    idx = fill(FlatGpuIndex(a.dim, metric=Metric.EUCLIDEAN, initial_size=a.rows, **TYPES[kind]), kind)
    for B in a.batches:
        q = queries[B] * (20 if kind == 'i8' else 1)
        for k in a.limits:
            compare(idx, 'table', kind, q, k, result)
            device_cases(idx, kind, idx._pre(q), k, result)
    del idx
    torch.cuda.empty_cache()
if a.cells:
    vq = VQCodec(a.cells, metric=Metric.EUCLIDEAN)
    vq._codebook = torch.randn((a.cells, a.dim), generator=torch.Generator(device=dev).manual_seed(1), device=dev).cpu().numpy()
    vq._is_trained = True
    idx = fill(IvfFlatGpuIndex(a.dim, vq_codec=vq, n_probe=a.probe, metric=Metric.EUCLIDEAN, initial_size=a.rows), 'f32')
    for B in a.batches:
        compare(idx, 'cells', 'f32', queries[B], a.limits[0], result)
result['all_answers_same'] = all(r['same_answer'] for r in result['search'])
result['wide_not_slower_anywhere'] = all(r['wide_not_slower'] for r in result['search'])
print("'wide' is not slower than 'host' in any case:", result['wide_not_slower_anywhere'], file=sys.stderr)
print(json.dumps(result))
