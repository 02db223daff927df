#!/usr/bin/env python3
"""Timings of the local correlation (include/sid_corr.h, libcorr) at Sentinel-1 size: a seeded 10000 x 10000 uint8 pair with
2 % zeros on device tensors, window 35, r alone as the output.  Workloads: the lattice at step 50 (the pattern-matching grid),
8 and 4, at step 1 on a 4000 x 4000 crop, and local_correlation_at on 40 000 scattered nodes.

Per workload: median / p10 / p90 / min / max in microseconds of --reps calls after warm-up, each between two device events on
the stream; the bytes the algorithm must move (both images once, the outputs once); the time of a device-to-device copy that
moves as many bytes in the same run (half of them read, half written) and the ratio to it; bit parity with the specification
(tests/corr_spec.py) on a 600 x 600 crop.  One condition on the design is measured and recorded: at step 8 the time at window
70 is less than 3 times the time at window 35 (a separable pass grows about 2 x, brute force per node about 4 x).
For contrast the specification's vectorised NumPy form (summed-area tables) on 2000 x 2000 on the host.
Without a GPU nothing is measured and the tool fails.

    python tools/local_corr_bench.py [--reps 20] [--size 10000] [--out profiles/local_corr_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sea_ice_drift_amd import libcorr           # noqa: E402
from tests import corr_spec                     # noqa: E402

WINDOW = 35


def stats(ts):
    ts = np.sort(np.asarray(ts))
    return dict(median=round(float(np.median(ts)), 1), p10=round(float(ts[int(0.1 * (len(ts) - 1))]), 1),
                p90=round(float(ts[int(round(0.9 * (len(ts) - 1)))]), 1), min=round(float(ts[0]), 1), max=round(float(ts[-1]), 1),
                reps=len(ts))


def timed(torch, call, reps, warm=3):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
        del out
    return stats(ts)


def copy_time(torch, nbytes, reps):
    """A device copy that moves `nbytes` in all: nbytes / 2 read and nbytes / 2 written."""
    src = torch.empty(max(nbytes // 2, 1), dtype=torch.uint8, device='cuda')
    dst = torch.empty_like(src)
    return timed(torch, lambda: dst.copy_(src), reps)


def host(t):
    return t.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--size', type=int, default=10000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('no GPU: nothing is measured without one')
    size, reps, w = args.size, max(args.reps, 20), WINDOW
    gen = torch.Generator(device='cuda').manual_seed(7)
    a = torch.randint(1, 256, (size, size), dtype=torch.uint8, device='cuda', generator=gen)
    b = torch.clamp(a.to(torch.float32) + 40.0 * torch.randn((size, size), device='cuda', generator=gen), 1, 255).to(torch.uint8)
    a[torch.rand((size, size), device='cuda', generator=gen) < 0.02] = 0
    b[torch.rand((size, size), device='cuda', generator=gen) < 0.02] = 0
    crop = min(4000, size)
    a1, b1 = a[:crop, :crop], b[:crop, :crop]                                   # (views: rows `size` bytes apart)
    npts = 40000
    pc = torch.randint(0, size, (npts,), dtype=torch.int32, device='cuda', generator=gen)
    pr = torch.randint(0, size, (npts,), dtype=torch.int32, device='cuda', generator=gen)
    k = min(600, size)
    ak, bk = host(a[:k, :k]), host(b[:k, :k])

    def lattice_parity(step, window=w):
        got = libcorr.local_correlation(a[:k, :k], b[:k, :k], window=window, step=step, return_count=True, return_sums=True)
        nr, nc = got[0].shape
        e = corr_spec.lattice(ak, bk, window, (window // 2, window // 2), (step, step), (nr, nc), (window * window + 1) // 2)
        return all(corr_spec.same_bits(host(g), e[key]) for g, key in zip(got, ('r', 'count', 'sums')))

    res = dict(device=torch.cuda.get_device_name(0), size=size, window=w, zeros=0.02, workloads=[])
    ok = True
    jobs = [('lattice step 50', a, b, 50), ('lattice step 8', a, b, 8), ('lattice step 4', a, b, 4),
            ('lattice step 1 on %d x %d' % (crop, crop), a1, b1, 1)]
    by_name = {}
    for name, ia, ib, step in jobs:
        t = timed(torch, lambda: libcorr.local_correlation(ia, ib, window=w, step=step), reps)
        nodes = ((ia.shape[0] - w) // step + 1) * ((ia.shape[1] - w) // step + 1)
        nbytes = 2 * ia.shape[0] * ia.shape[1] + 8 * nodes
        tc = copy_time(torch, nbytes, reps)
        wl = dict(name=name, nodes=nodes, time_us=t, bytes=dict(images=2 * ia.shape[0] * ia.shape[1], outputs=8 * nodes, total=nbytes),
                  copy_us=tc, ratio_to_copy=round(t['median'] / tc['median'], 2), parity=lattice_parity(step))
        ok = ok and wl['parity']
        res['workloads'].append(wl)
        by_name[name] = wl
    t = timed(torch, lambda: libcorr.local_correlation_at(a, b, pc, pr, window=w), reps)
    nbytes = 2 * size * size + 8 * npts + 8 * npts
    tc = copy_time(torch, nbytes, reps)
    kc, kr = pc % k, pr % k
    got = libcorr.local_correlation_at(a[:k, :k], b[:k, :k], kc, kr, window=w, return_count=True, return_sums=True)
    e = corr_spec.points(ak, bk, w, host(kc), host(kr), None, (w * w + 1) // 2)
    parity = all(corr_spec.same_bits(host(g), e[key]) for g, key in zip(got, ('r', 'count', 'sums')))
    ok = ok and parity
    res['workloads'].append(dict(name='local_correlation_at, %d scattered nodes' % npts, nodes=npts, time_us=t,
                                 bytes=dict(images=2 * size * size, centres=8 * npts, outputs=8 * npts, total=nbytes,
                                            note='both images counted whole, as for the lattice; the windows touch %d bytes'
                                                 % (2 * npts * w * w)),
                                 copy_us=tc, ratio_to_copy=round(t['median'] / tc['median'], 2), parity=parity))
    # the design condition: a separable pass, not brute force per node
    t35 = by_name['lattice step 8']['time_us']
    t70 = timed(torch, lambda: libcorr.local_correlation(a, b, window=2 * w, step=8), reps)
    ratio = t70['median'] / t35['median']
    res['window_growth'] = dict(step=8, window_35_us=t35, window_70_us=t70, ratio=round(ratio, 3), bar=3.0, met=bool(ratio < 3.0),
                                parity_window_70=lattice_parity(8, 2 * w))
    ok = ok and res['window_growth']['parity_window_70']
    # host contrast
    hs = min(2000, size)
    ah, bh = host(a[:hs, :hs]), host(b[:hs, :hs])
    contrast = []
    for step in (8, 1):
        n = (hs - w) // step + 1
        t0 = time.perf_counter()
        corr_spec.lattice(ah, bh, w, (w // 2, w // 2), (step, step), (n, n), (w * w + 1) // 2)
        contrast.append(dict(size=hs, step=step, nodes=n * n, seconds=round(time.perf_counter() - t0, 3)))
    res['host_contrast_numpy'] = contrast
    res['ok'] = bool(ok)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0 if ok and res['window_growth']['met'] else 1


if __name__ == '__main__':
    sys.exit(main())
