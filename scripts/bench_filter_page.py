#!/usr/bin/env python3
"""Pages of the document listing: what ``annlite_order_page`` / ``annlite_bitmap_page`` cost, and what they
save ``AnnLite.filter()`` end to end.

    python scripts/bench_filter_page.py                      # tables on stderr, one JSON line on stdout

Three columns -- ``a`` int, ``f`` float, ``s`` str, 100 values each, each missing in a few percent of the rows --, the one-leaf filter
``a < 50`` (about half the rows) or no filter, pages of 10 rows.

Kernels alone (``--rows``, default 1M and 10M): ONE pair of device events around ``--launches`` back-to-back calls (each a memset, one
launch per digit, a collect and a sort on one stream), over their number; the median of ``--reps`` windows after a warm-up.  ``bytes``:
what a call must read, from the shapes -- per launch that reads the column (the digits and the collect) the mask words, the
row-present words, the column's present words and its 8-byte (str: 4-byte) values of every row; the unordered page reads the bitmaps
alone.  ``share``: bytes over that time against the HBM peak of 8.0 TB/s.  The column of the previous launch may still sit in the
Infinity Cache (256 MB; 10M rows of one column are 80 MB).  The 10M-row store is the 1M-row store's arrays repeated on the device.

End to end (``--e2e-rows``, default 1M): ``ann.filter(f, limit=10, offset=o, order_by=c)`` for every ``o`` of ``--offsets`` and ``c`` in
none / ``a`` / ``s``, with the filter and without; two facades over the same rows in one process, ``filter_eval='auto'`` (mask and page
on the device) and ``filter_eval='host'`` (``filter.select`` over the tags, then Python's ``sorted`` over the selected rows: what the
release before the pages did once its mask was made, plus its host mask), alternating; a host clock around the call, which ends in the
page's copy to the host.  After one warm-up pair the pair is timed ``--e2e-reps`` times (default 2: the spread of a case is the
distance between its two runs); a case counts as won where the device's slowest run beats the host's fastest.
"""
import argparse
import json
import math
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
p.add_argument('--offsets', type=int, nargs='+', default=[0, 1000, 500_000])
p.add_argument('--e2e-rows', type=int, default=1_000_000)
p.add_argument('--e2e-reps', type=int, default=2)
p.add_argument('--dim', type=int, default=8)
a = p.parse_args()
assert a.launches >= 100 and a.e2e_reps >= 2
torch.cuda.set_device(0)
dev = torch.device('cuda', 0)

WORDS = ['w%02d' % ((j * 37) % 100) for j in range(100)]  # (the dictionary's order is not the sorted order)
COLUMNS = [('a', int), ('f', float), ('s', str)]
FILTER = {'a': {'$lt': 50}}
LIMIT = 10


def make_tags(n, seed=0):
    rs = np.random.RandomState(seed)
    av, fv, sv = rs.randint(0, 100, n).tolist(), (rs.randint(0, 100, n) / 4).tolist(), rs.randint(0, len(WORDS), n).tolist()
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


def call_shape(st, column, masked):
    """(launches that read the rows, bytes they must read): one launch per digit that can differ, and the collect"""
    n = len(st)
    row_digits = max(1, math.ceil(math.log(n, 256)))
    bitmaps = (2 if masked else 1) * (n // 8)
    if column is None:
        return row_digits + 1, (row_digits + 1) * bitmaps
    kind = st.kinds[column]
    key_digits = (1 if len(st.dictionary(column)) <= 256 else 2) if kind == CODE else 8
    launches = 1 + key_digits + row_digits + 1
    return launches, launches * (bitmaps + n // 8 + n * (4 if kind == CODE else 8))


def kernel_time(st, mask, column, first):
    """seconds per call, back to back on the stream"""
    ws = ops.ScanWorkspace()
    out = torch.empty((LIMIT + 1,), dtype=torch.int32, device=dev)
    words = None if mask is None else mask.words_for(st.n_words)

    def call():
        if column is None:
            bits, and_bits = (st.rows, None) if words is None else (words, st.rows)
            ops.bitmap_page(bits, len(st), st.n_words, first, LIMIT, and_bits=and_bits, out=out, workspace=ws)
        else:
            kind = st.kinds[column]
            ops.order_page(words, st.rows, st.values[column], kind, st.present[column], len(st), st.n_words, False, first, LIMIT,
                           rank=st._rank(column) if kind == CODE else None, out=out, workspace=ws)

    def window():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.launches):
            call()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.launches * 1e-3

    for _ in range(20):
        call()
    torch.cuda.synchronize()
    return float(np.median([window() for _ in range(a.reps)])), int(out[LIMIT].item())


result = {'kernel': [], 'e2e': []}
base_n = min(1_000_000, max(a.rows + [a.e2e_rows])) // 32 * 32
t0 = time.time()
tags = make_tags(max(base_n, a.e2e_rows))
base = ColumnStore(COLUMNS)
base.append(tags[:base_n])
print('tags + base store of %d rows: %.1f s' % (base_n, time.time() - t0), file=sys.stderr)
print('%10s %7s %6s %8s %9s %10s %10s %8s' % ('rows', 'filter', 'order', 'first', 'launches', 'call us', 'MB', 'share'), file=sys.stderr)
for n in a.rows:
    st = base if n == len(base) else repeated(base, n)
    mask = st.evaluate(st.compile(FILTER))
    for masked in (True, False):
        for column in (None, 'a', 'f', 's'):
            for first in a.offsets:
                launches, nbytes = call_shape(st, column, masked)
                sec, rows = kernel_time(st, mask if masked else None, column, first)
                row = dict(rows=len(st), filter=masked, selected=len(mask) if masked else None, order_by=column, first=first, page_rows=rows,
                           launches=launches, call_us=sec * 1e6, bytes=nbytes, share_of_hbm_peak=nbytes / sec / HBM_PEAK)
                result['kernel'].append(row)
                print('%10d %7s %6s %8d %9d %10.1f %10.2f %8.3f' % (len(st), 'a<50' if masked else '-', column or '-', first, launches, sec * 1e6,
                                                                   nbytes / 1e6, row['share_of_hbm_peak']), file=sys.stderr)
    del st, mask

# ---- end to end
n = a.e2e_rows
rs = np.random.RandomState(1)
x = rs.randn(n, a.dim).astype(np.float32)
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
    print('%10s %7s %6s %8s %24s %24s %8s %5s' % ('rows', 'filter', 'order', 'offset', 'device ms (each run)', 'host ms (each run)', 'ratio', 'won'),
          file=sys.stderr)
    for flt in (FILTER, None):
        for column in (None, 'a', 's'):
            for offset in a.offsets:
                times = {'auto': [], 'host': []}
                answers = {}
                for rep in range(a.e2e_reps + 1):
                    for mode, ann in anns.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        answers[mode] = [d.id for d in ann.filter(flt, limit=LIMIT, offset=offset, order_by=column)]
                        dt = time.perf_counter() - t0
                        if rep:
                            times[mode].append(dt)
                assert anns['auto'].last_filter_page == 'gpu' and anns['host'].last_filter_page == 'host'
                assert answers['auto'] == answers['host'], (flt, column, offset)
                won = max(times['auto']) < min(times['host'])
                result['e2e'].append(dict(rows=n, filter=flt is not None, order_by=column, offset=offset, page_rows=len(answers['auto']),
                                          device_ms=[t * 1e3 for t in times['auto']], host_ms=[t * 1e3 for t in times['host']], won=won))
                print('%10d %7s %6s %8d %24s %24s %8.0f %5s' % (n, 'a<50' if flt else '-', column or '-', offset,
                                                              ' '.join('%.3f' % (t * 1e3) for t in times['auto']),
                                                              ' '.join('%.1f' % (t * 1e3) for t in times['host']),
                                                              np.median(times['host']) / np.median(times['auto']), won), file=sys.stderr)
print(json.dumps(result))
