#!/usr/bin/env python3
"""Filterable columns: what ``annlite_filter_eval`` costs, and what it saves a filtered search end to end.

    python scripts/bench_filter_eval.py                      # a table on stderr, one JSON line on stdout

Three columns -- ``a`` int, ``f`` float, ``s`` str with 100 values, each missing in a few percent of the rows -- and filters of 1, 3
and 8 leaves.

Kernel (``--rows``, default 1M and 10M): device events over ``--launches`` launches after a warm-up, the median of ``--reps`` windows.
Three figures per launch: ``stream`` -- ONE pair of events around the whole window of back-to-back launches, over their number (the
kernel plus what a dependent launch costs on the stream, or the host's enqueue rate where that is the slower; the columns of the
previous launch may still sit in the Infinity Cache -- 256 MB, where 10M rows x 3 columns are 200 MB); ``warm`` -- a pair of events
around EVERY launch, summed (adds what the two event records cost per launch); ``cold`` -- the same with ``--flush-mb`` of other
memory written between the launches, outside the events.  ``bytes``: what a launch must read and write, from the shapes -- per
referenced column 8 B (4 B for str) and one present bit per row, one row-present bit and one output bit per row; ``share``: bytes
over the ``stream`` / ``cold`` time against the HBM peak of 8.0 TB/s (the achievable copy rate on this part is about 6.3 TB/s).
The 10M-row store is the 1M-row store's arrays repeated on the device (same values, same dictionary).

End to end (``--e2e-rows``, default 1M): ``AnnLite.search_numpy(filter=...)`` on a ``FlatGpuIndex`` of dimension ``--dim``, a batch of
``--batch`` queries, limit 10; two facades over the same rows, ``filter_eval='auto'`` (the filter evaluated on the device) and
``filter_eval='host'`` (``filter.select`` over the tags: what every release before the columns did), alternating, wall clock around
the call (which ends in the copy of the answer to the host); the median of ``--e2e-reps`` calls each, after one warm-up call each.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from annlite_amd import AnnLite, ops  # noqa: E402
from annlite_amd.columns import CODE, ColumnStore  # noqa: E402
from annlite_amd.index import Document, DocumentArray  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s: the part's specification

p = argparse.ArgumentParser()
p.add_argument('--rows', type=int, nargs='+', default=[1_000_000, 10_000_000])
p.add_argument('--launches', type=int, default=200)
p.add_argument('--reps', type=int, default=3)
p.add_argument('--flush-mb', type=int, default=1024)
p.add_argument('--e2e-rows', type=int, default=1_000_000)
p.add_argument('--e2e-reps', type=int, default=3)
p.add_argument('--dim', type=int, default=32)
p.add_argument('--batch', type=int, default=64)
a = p.parse_args()
assert a.launches >= 100
torch.cuda.set_device(0)
dev = torch.device('cuda', 0)

WORDS = ['w%02d' % j for j in range(100)]
COLUMNS = [('a', int), ('f', float), ('s', str)]
FILTERS = {
    1: {'a': {'$lt': 500}},
    3: {'a': {'$gte': 100}, 'f': {'$lt': 0.5}, 's': {'$in': WORDS[:10]}},
    8: {'$or': [{'a': {'$lt': 50}, 'f': {'$gt': 0.25}}, {'a': {'$in': [7, 77, 777]}, 's': {'$lt': 'w50'}},
                {'f': {'$gte': 0.9}, 's': {'$neq': 'w00'}, 'a': {'$gte': 900}, '$not': {'f': {'$lt': 0.95}}}]},
}


def make_tags(n, seed=0):
    rs = np.random.RandomState(seed)
    av, fv, sv = rs.randint(0, 1000, n).tolist(), rs.rand(n).tolist(), rs.randint(0, len(WORDS), n).tolist()
    miss = rs.randint(0, 32, n).tolist()
    tags = []
    for r in range(n):
        t = {}
        if miss[r] != 0:
            t['a'] = av[r]
        if miss[r] != 1:
            t['f'] = fv[r]
        if miss[r] != 2:
            t['s'] = WORDS[sv[r]]
        tags.append(t)
    return tags


def repeated(base, n):
    """a store of n rows: the base store's arrays repeated on the device"""
    st = ColumnStore(COLUMNS)
    times = -(-n // len(base))
    st._grow(times * len(base))
    m, mw = len(base), len(base) // 32
    assert m % 32 == 0
    for j in range(times):
        for name in st.kinds:
            st.values[name][j * m:(j + 1) * m] = base.values[name][:m]
            st.present[name][j * mw:(j + 1) * mw] = base.present[name][:mw]
        st.rows[j * mw:(j + 1) * mw] = base.rows[:mw]
    st._codes = base._codes
    st._n = times * m
    return st


def launch_bytes(st, prog):
    cols = {leaf.column for leaf in prog.leaves}
    n = len(st)
    return sum(n * (4 if st.kinds[c] == CODE else 8) + n // 8 for c in cols) + 2 * (n // 8)


def kernel_times(st, prog, flush):
    """(stream, warm, cold) seconds per launch"""
    P, keep = st.bind(prog)
    out = torch.empty((st.n_words,), dtype=torch.int32, device=dev)
    count = torch.zeros((1,), dtype=torch.int64, device=dev)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]

    def window(cold):
        for s, e in ev:
            if cold:
                flush.add_(1)
            s.record()
            ops.filter_eval(P, len(st), st.n_words, and_bits=st.rows, out=out, count=count)
            e.record()
        torch.cuda.synchronize()
        return sum(s.elapsed_time(e) for s, e in ev) / len(ev) * 1e-3

    def stream():
        s, e = ev[0]
        s.record()
        for _ in range(a.launches):
            ops.filter_eval(P, len(st), st.n_words, and_bits=st.rows, out=out, count=count)
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.launches * 1e-3

    for _ in range(20):
        ops.filter_eval(P, len(st), st.n_words, and_bits=st.rows, out=out, count=count)
    torch.cuda.synchronize()
    return (float(np.median([stream() for _ in range(a.reps)])), float(np.median([window(False) for _ in range(a.reps)])),
            float(np.median([window(True) for _ in range(a.reps)])))


result = {'kernel': [], 'e2e': []}
base_n = min(1_000_000, max(a.rows + [a.e2e_rows])) // 32 * 32
t0 = time.time()
tags = make_tags(max(base_n, a.e2e_rows))
base = ColumnStore(COLUMNS)
base.append(tags[:base_n])
print('tags + base store of %d rows: %.1f s' % (base_n, time.time() - t0), file=sys.stderr)
flush = torch.zeros((a.flush_mb * (1 << 20) // 4,), dtype=torch.int32, device=dev)
print('%10s %6s %10s %10s %10s %10s %13s %12s' % ('rows', 'leaves', 'stream us', 'warm us', 'cold us', 'MB', 'stream share', 'cold share'),
      file=sys.stderr)
for n in a.rows:
    st = base if n == len(base) else repeated(base, n)
    for leaves, flt in FILTERS.items():
        prog = st.compile(flt)
        assert prog is not None and len(prog.leaves) == leaves
        selected = len(st.evaluate(prog))
        stream_s, warm, cold = kernel_times(st, prog, flush)
        nbytes = launch_bytes(st, prog)
        row = dict(rows=len(st), leaves=leaves, columns=len({leaf.column for leaf in prog.leaves}), selected=selected, stream_us=stream_s * 1e6,
                   warm_us=warm * 1e6, cold_us=cold * 1e6, bytes=nbytes, stream_share_of_hbm_peak=nbytes / stream_s / HBM_PEAK,
                   cold_share_of_hbm_peak=nbytes / cold / HBM_PEAK)
        result['kernel'].append(row)
        print('%10d %6d %10.1f %10.1f %10.1f %10.2f %13.3f %12.3f' % (len(st), leaves, stream_s * 1e6, warm * 1e6, cold * 1e6, nbytes / 1e6,
                                                                  row['stream_share_of_hbm_peak'], row['cold_share_of_hbm_peak']), file=sys.stderr)
    del st
del flush

# ---- end to end
n = a.e2e_rows
rs = np.random.RandomState(1)
x = rs.randn(n, a.dim).astype(np.float32)
q = rs.randn(a.batch, a.dim).astype(np.float32)
with tempfile.TemporaryDirectory() as tmp:
    anns = {}
    t0 = time.time()
    for mode in ('auto', 'host'):
        ann = AnnLite(a.dim, metric='euclidean', data_path=os.path.join(tmp, mode), columns=COLUMNS, filter_eval=mode)
        for lo in range(0, n, 100_000):
            hi = min(n, lo + 100_000)
            ann.index(DocumentArray([Document(id=str(r), embedding=x[r], tags=tags[r]) for r in range(lo, hi)]))
        anns[mode] = ann
    print('two facades of %d rows: %.1f s' % (n, time.time() - t0), file=sys.stderr)
    print('%10s %6s %12s %12s %8s' % ('rows', 'leaves', 'device ms', 'host ms', 'ratio'), file=sys.stderr)
    for leaves, flt in FILTERS.items():
        times = {'auto': [], 'host': []}
        answers = {}
        for rep in range(a.e2e_reps + 1):
            for mode, ann in anns.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                answers[mode] = ann.search_numpy(q, filter=flt, limit=10)
                dt = time.perf_counter() - t0
                if rep:
                    times[mode].append(dt)
        assert anns['auto'].last_filter_eval == 'gpu' and anns['host'].last_filter_eval == 'host'
        assert all(np.array_equal(u, v) for u, v in zip(answers['auto'][1], answers['host'][1]))
        dev_s, host_s = float(np.median(times['auto'])), float(np.median(times['host']))
        result['e2e'].append(dict(rows=n, leaves=leaves, batch=a.batch, dim=a.dim, device_ms=dev_s * 1e3, host_ms=host_s * 1e3))
        print('%10d %6d %12.2f %12.2f %8.0f' % (n, leaves, dev_s * 1e3, host_s * 1e3, host_s / dev_s), file=sys.stderr)
print(json.dumps(result))
