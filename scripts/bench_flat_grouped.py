#!/usr/bin/env python3
"""A filter per query in one batch ("a filter per query"): ``search_batch_grouped`` against the loop of
single-filter ``search_batch`` calls it replaces, with one unfiltered call as the floor.

    python scripts/bench_flat_grouped.py                   # tables on stderr, one JSON line on stdout

Shape (``--rows`` x ``--dim``, default 1M x 128; ``k = 10``; batches of ``--batches``, default 1024 and 64; row types f32, f16, int8):
one ``FlatGpuIndex`` per row type, EUCLIDEAN, i.i.d. normal rows made on the device.  Filters: a ``ColumnStore`` with one integer column
``tenant`` (uniform in [0, 1000)) and, per case, ``--groups`` (default 2, 8, 64) DISTINCT range filters ``lo <= tenant < lo + 1000 share``
keeping ``--shares`` (default 50 %, 10 %, 1 %) of the rows each, every one compiled and evaluated on the device once per case
(``annlite_filter_eval``: what a facade call does per distinct filter); the queries are dealt to the groups round-robin.

Per case three things ALTERNATE in one process, a warm-up each, then two timings each; a timing is the host clock around ``--calls``
whole calls, ending in a device synchronise:
  (a) grouped  ``search_batch_grouped(q, k, masks, group_of)``: the mask tensor is built inside the call
  (b) looped   one ``search_batch(q[group g], k, indices=mask g)`` per group: what a caller does without (a); code (a) does not touch
  (c) floor    one unfiltered ``search_batch(q, k)``
``spread``: the largest difference between the two timings of any of the three; (a) counts as faster where the slower of its timings
beats the faster of (b)'s by more than that.  The answers of (a) and (b) are compared on every case.

Kernel alone, by device events around ``--launches`` back-to-back calls after a warm-up (the median of ``--reps`` windows):
``grouped_kernel_ms`` -- ``ops.flat_search_topk_grouped`` over the prebuilt mask tensor -- and ``floor_kernel_ms`` -- the row type's
ungrouped ``flat_search_topk``; ``eval_ms``: one ``annlite_filter_eval`` of one of the case's filters, the same way.
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
from annlite_amd.columns import ColumnStore  # noqa: E402
from annlite_amd.core.index.flat_gpu import FlatGpuIndex  # noqa: E402
from annlite_amd.enums import Metric  # noqa: E402

p = argparse.ArgumentParser()
p.add_argument('--rows', type=int, default=1_000_000)
p.add_argument('--dim', type=int, default=128)
p.add_argument('--batches', type=int, nargs='+', default=[1024, 64])
p.add_argument('--groups', type=int, nargs='+', default=[2, 8, 64])
p.add_argument('--shares', type=float, nargs='+', default=[0.5, 0.1, 0.01])
p.add_argument('--types', nargs='+', default=['f32', 'f16', 'i8'])
p.add_argument('--calls', type=int, default=5)
p.add_argument('--launches', type=int, default=20)
p.add_argument('--reps', type=int, default=3)
a = p.parse_args()
torch.cuda.set_device(0)
dev = torch.device('cuda', 0)
K = 10
TENANTS = 1000
TYPES = {'f32': dict(), 'f16': dict(dtype=np.float16), 'i8': dict(dtype=np.int8)}


def make_index(kind, n):
    idx = FlatGpuIndex(a.dim, metric=Metric.EUCLIDEAN, initial_size=n, **TYPES[kind])
    g = torch.Generator(device=dev).manual_seed(1)
    for lo in range(0, n, 1_000_000):
        hi = min(n, lo + 1_000_000)
        x = torch.randn((hi - lo, a.dim), generator=g, device=dev)
        idx.add_with_ids(x * 20 if kind == 'i8' else x, torch.arange(lo, hi, device=dev))  # (int8: codes of a few dozen steps)
    return idx


def make_columns(n):
    tenant = np.random.RandomState(2).randint(0, TENANTS, size=n)
    store = ColumnStore([('tenant', int)], device=dev, initial_capacity=n)
    store.append([{'tenant': int(t)} for t in tenant])
    return store


def filters_of(G, share):
    """G distinct ranges of the same width over the tenants"""
    width = max(1, int(round(share * TENANTS)))
    los = np.unique(np.linspace(0, TENANTS - width, G).astype(int))
    assert len(los) == G, 'the ranges are not distinct'
    return [{'tenant': {'$gte': int(lo), '$lt': int(lo) + width}} for lo in los]


def events(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    for _ in range(a.reps):
        s.record()
        for _ in range(a.launches):
            fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) / a.launches)
    return float(np.median(times))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.calls):
        ans = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / a.calls, ans


def cases(kind, store, result):
    n = a.rows
    idx = make_index(kind, n)
    tag, scale = idx._kind.tag, idx._i8_scale or 1.0
    g = torch.Generator(device=dev).manual_seed(3)
    for B in a.batches:
        q = torch.randn((B, a.dim), generator=g, device=dev) * (20 if kind == 'i8' else 1)
        for G in a.groups:
            if G > B:
                continue
            group_of = np.arange(B) % G  # round-robin
            at = [torch.as_tensor(np.flatnonzero(group_of == gi), device=dev) for gi in range(G)]
            qs = [q[i].contiguous() for i in at]
            for share in a.shares:
                programs = [store.compile(f) for f in filters_of(G, share)]
                assert all(pr is not None for pr in programs)
                masks = [store.evaluate(pr) for pr in programs]
                n_sel = [len(m) for m in masks]

                def grouped():
                    return idx.search_batch_grouped(q, limit=K, selections=masks, group_of=group_of)

                def looped():
                    d = torch.empty((B, K), dtype=torch.float32, device=dev)
                    i = torch.empty((B, K), dtype=torch.int64, device=dev)
                    for gi in range(G):
                        d[at[gi]], i[at[gi]] = idx.search_batch(qs[gi], limit=K, indices=masks[gi])
                    return d, i

                def floor():
                    return idx.search_batch(q, limit=K)

                t = {'grouped': [], 'looped': [], 'floor': []}
                ans = {}
                for rep in range(3):  # (a warm-up, then the two timings)
                    for name, fn in (('grouped', grouped), ('looped', looped), ('floor', floor)):
                        dt, ans[name] = wall(fn)
                        if rep:
                            t[name].append(dt)
                assert idx.last_filter_batch == 'grouped'
                same = torch.equal(ans['grouped'][1], ans['looped'][1]) and torch.equal(ans['grouped'][0].view(torch.int32),
                                                                                        ans['looped'][0].view(torch.int32))
                spread = max(abs(v[0] - v[1]) for v in t.values())
                stack = torch.stack([idx._filter_bits(m) for m in masks]).contiguous()
                group_dev = torch.as_tensor(group_of.astype(np.int32), device=dev)
                grouped_kernel = events(lambda: ops.flat_search_topk_grouped(tag, 1, q, idx._vectors, idx._norms, stack, group_dev, K, valid_bits=idx._valid,
                                                                             n_rows=n, scale=scale, sqrt=True, workspace=idx._ws))
                overflowed = ops.flat_overflow_count(idx._ws)
                floor_kernel = events(lambda: idx._kind.topk(1, q, idx._vectors, idx._norms, K, valid_bits=idx._valid, n_rows=n, sqrt=True,
                                                             workspace=idx._ws))
                eval_ms = events(lambda: store.evaluate(programs[0]))
                row = dict(type=kind, rows=n, dim=a.dim, batch=B, groups=G, share=share, n_sel_mean=float(np.mean(n_sel)),
                           grouped_ms=[v * 1e3 for v in t['grouped']], looped_ms=[v * 1e3 for v in t['looped']],
                           floor_ms=[v * 1e3 for v in t['floor']], spread_ms=spread * 1e3,
                           grouped_faster=bool(max(t['grouped']) + spread < min(t['looped'])),
                           looped_faster=bool(max(t['looped']) + spread < min(t['grouped'])), same_answer=bool(same),
                           speedup=min(t['looped']) / min(t['grouped']), grouped_kernel_ms=grouped_kernel, floor_kernel_ms=floor_kernel,
                           eval_ms=eval_ms, overflowed=int(overflowed))
                result['search'].append(row)
                print('%4s %5d %3d %5.2f  grouped %8.3f %8.3f  looped %8.3f %8.3f  floor %7.3f %7.3f  spread %6.3f  %6.2fx %-7s  kernel %7.3f / %7.3f  '
                      'eval %6.3f  ovf %d %s' % (kind, B, G, share, *row['grouped_ms'], *row['looped_ms'], *row['floor_ms'], row['spread_ms'],
                                                 row['speedup'], 'grouped' if row['grouped_faster'] else 'looped' if row['looped_faster'] else '-',
                                                 grouped_kernel, floor_kernel, eval_ms, overflowed, '' if same else 'ANSWERS DIFFER'),
                      file=sys.stderr, flush=True)
                del masks, stack
    del idx
    torch.cuda.empty_cache()


result = {'search': []}
print('type batch   G share  ms per call, two timings each; kernel: grouped / ungrouped unfiltered, by device events', file=sys.stderr)
store = make_columns(a.rows)
for kind in a.types:
    cases(kind, store, result)
result['all_answers_same'] = all(r['same_answer'] for r in result['search'])
print(json.dumps(result))
