#!/usr/bin/env python
"""The coarse quantiser's two assignment paths side by side: ``ivf_select_cells`` with one probe ('chain') and
``annlite_vq_assign`` ('mfma'), alternating in one process on the same seeded inputs, device events around every call.

    python scripts/bench_vq_assign.py --n 1000000,10000000 --d 128,768 --c 256,1024,4096 --data clustered,normal
    python scripts/bench_vq_assign.py --lloyd            # one Lloyd iteration of VQCodec.fit at 1M x 128, C = 1024, and k-means++'s share
    python scripts/bench_vq_assign.py --fit-spread       # seeded fits on 4096 x 16, C = 32: inertia of 'mfma' against 'chain' (no timing)

One JSON line per case: the median time of each path, the undecided share of 'mfma', the contraction's rate (2 N C D FLOP over the
call), and whether the two answers were equal (they must be).  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from annlite_amd import ops  # noqa: E402
from annlite_amd.core.codec.vq import VQCodec  # noqa: E402


def make(kind: str, N: int, D: int, C: int, seed: int = 0):
    """(rows, centroids) on the device: i.i.d. normal rows, or rows around 4096 normal centres; the centroids are C of the rows"""
    gen = torch.Generator(device=ops.device())
    gen.manual_seed(seed)
    x = torch.randn((N, D), generator=gen, device=ops.device(), dtype=torch.float32)
    if kind == 'clustered':
        centres = 3.0 * torch.randn((4096, D), generator=gen, device=ops.device(), dtype=torch.float32)
        pick = torch.randint(0, 4096, (N,), generator=gen, device=ops.device())
        step = 1 << 20
        for b in range(0, N, step):  # (in slices: the gathered centres of 10M x 768 would be a second table)
            x[b:b + step] += centres[pick[b:b + step]]
    cb = x[torch.randperm(N, generator=gen, device=ops.device())[:C]].clone()
    return x, cb


def timed(fn, reps: int):
    """median and spread (min, max) in ms of ``reps`` calls, each between two device events"""
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def alternate(paths: dict, reps: int):
    """{name: (median, min, max) ms}: one warm-up of every path, then ``reps`` rounds that run the paths in turn"""
    for fn in paths.values():
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in paths}
    for _ in range(reps):
        for k, fn in paths.items():
            ts[k].append(timed(fn, 1)[0])
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ts.items()}


def bench_assign(kind: str, N: int, D: int, C: int, reps: int) -> dict:
    x, cb = make(kind, N, D, C)
    ws = ops.ScanWorkspace()
    out = {}
    paths = {'chain': lambda: out.__setitem__('chain', ops.ivf_select_cells(0, x, cb, 1)),
             'mfma': lambda: out.__setitem__('mfma', ops.vq_assign(x, cb, ws))}
    t = alternate(paths, reps)
    equal = bool(torch.equal(out['chain'][:, 0], out['mfma']))
    undecided = ops.vq_assign_undecided(ws)
    return dict(bench='assign', data=kind, N=N, D=D, C=C, reps=reps, chain_ms=t['chain'], mfma_ms=t['mfma'],
                speedup=t['chain'][0] / t['mfma'][0], undecided=undecided, undecided_share=undecided / N,
                mfma_call_tflops=2.0 * N * C * D / (t['mfma'][0] * 1e-3) / 1e12, equal=equal)


def bench_lloyd(N: int, D: int, C: int, reps: int) -> dict:
    x, cb = make('clustered', N, D, C)
    codecs = {}
    for path in ('chain', 'mfma'):
        codecs[path] = VQCodec(C)
        codecs[path].assign = path
    t = alternate({k: (lambda c=c: c._lloyd_step(x, cb)) for k, c in codecs.items()}, reps)
    gen = torch.Generator(device=x.device)
    gen.manual_seed(0)
    seed_ms = timed(lambda: VQCodec._kmeanspp(x, C, gen), 1)[0]
    it = codecs['mfma'].iter
    return dict(bench='lloyd', N=N, D=D, C=C, reps=reps, chain_ms=t['chain'], mfma_ms=t['mfma'], speedup=t['chain'][0] / t['mfma'][0],
                kmeanspp_ms=seed_ms, kmeanspp_share_of_restart_mfma=seed_ms / (seed_ms + it * t['mfma'][0]),
                kmeanspp_share_of_restart_chain=seed_ms / (seed_ms + it * t['chain'][0]))


def fit_spread(seed: int, repeats: int = 5) -> dict:
    """Seeded ``VQCodec.fit`` on the 4096 x 16, C = 32 table of tests/test_vq_assign_gpu.py: the float64 inertia of ``repeats`` 'chain'
    fits (their run-to-run spread: f32 atomics in arrival order) and of one 'mfma' fit, as relative differences."""
    rs = np.random.RandomState(5)
    x = (rs.randn(32, 16)[rs.randint(0, 32, 4096)] * 3.0 + rs.randn(4096, 16)).astype(np.float32)

    def inertia(path):
        codec = VQCodec(32, iter=25, n_init=2)
        codec.seed, codec.assign = seed, path
        codec.fit(x)
        cb = codec.codebook.astype(np.float64)
        return float(((x[:, None, :] - cb[None]) ** 2).sum(2).min(1).sum())

    chain = [inertia('chain') for _ in range(repeats)]
    mfma = inertia('mfma')
    mean = float(np.mean(chain))
    return dict(bench='fit_spread', seed=seed, chain_inertia=['%.17g' % v for v in chain], mfma_inertia='%.17g' % mfma,
                chain_spread='%.3e' % ((max(chain) - min(chain)) / mean), mfma_minus_chain='%.3e' % ((mfma - mean) / mean),
                mfma_minus_chain_max='%.3e' % ((mfma - min(chain)) / mean))


def main():
    ints = lambda s: [int(v) for v in s.split(',')]  # noqa: E731
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=ints, default=[1000000, 10000000])
    ap.add_argument('--d', type=ints, default=[128, 768])
    ap.add_argument('--c', type=ints, default=[256, 1024, 4096])
    ap.add_argument('--data', type=lambda s: s.split(','), default=['clustered', 'normal'])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--lloyd', action='store_true')
    ap.add_argument('--fit-spread', action='store_true')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a GPU'

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    if args.fit_spread:
        for seed in (1234, 1, 2):
            emit(fit_spread(seed))
        return
    if args.lloyd:
        emit(bench_lloyd(1000000, 128, 1024, args.reps))
        return
    for N in args.n:
        for D in args.d:
            for kind in args.data:
                for C in args.c:
                    emit(bench_assign(kind, N, D, C, args.reps))


if __name__ == '__main__':
    main()
