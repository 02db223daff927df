#!/usr/bin/env python3
"""Timings of the sigma0 preparation (sea_ice_drift_amd.lib.prepare_image, include/sid_prep.h) on a 10000 x 10000 float32 scene,
device tensors in and out, HIP events on the stream, median of --reps calls after warm-up:

  a_uint8_ms        get_uint8_image alone (percentiles + scaling of an image already in dB): the staging step as it was
  b_db_ms           prepare_image, dB only
  c_full_ms         prepare_image with HH correction, mask and detrend (the host's fit of ~40 000 samples included)
  apply_db_ms / apply_full_ms / subsample_ms / spatial_mean_ms     the new passes alone
  bound_*_ms        bytes moved / 6.29 TB/s (the measured float4 copy rate of the MI355X); for b and c: a_uint8_ms plus the
                    apply pass's bytes at that rate
  host_numpy_*_s    the NumPy restatement of the same chains on this host (one run each; --no-host skips them)
Kernel times alone: run under `rocprofv3 --kernel-trace --stats` (kernels apply_kernel<...>, subsample_kernel, mean_kernel).

    python tools/prep_bench.py [--size 10000] [--reps 20] [--out FILE] [--no-host]
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sea_ice_drift_amd import _capi, lib                   # noqa: E402

COPY_RATE = 6.29e12                                        # bytes / s, float4 copy on the MI355X
FACTOR = -0.27


def scene(n, device):
    import torch
    g = torch.Generator(device=device).manual_seed(7)
    c = torch.arange(n, device=device, dtype=torch.float32)[None, :]
    db = -18.0 - 9.0 * c / n + 4.0 * torch.randn((n, n), device=device, generator=g)
    lin = torch.pow(10.0, db / 10.0)
    u = torch.rand((n, n), device=device, generator=g)
    lin[u < 0.02] = float('nan')
    lin[(u >= 0.02) & (u < 0.025)] = 0.0
    lin[:, :30] = 0.0
    ia = (20.0 + 26.0 * c / n).expand(n, n).contiguous()
    mask = torch.zeros((n, n), dtype=torch.bool, device=device)
    mask[n // 3: n // 3 + n // 10, n // 5: n // 2] = True
    del db, u
    return lin, ia, mask


def events_ms(fn, reps, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def numpy_mean(shape, x):
    cols, rows = np.meshgrid(np.arange(0, shape[1]), np.arange(0, shape[0]))
    img2 = x[0] * cols
    img2 += x[1] * cols ** 2
    img2 += x[2] * rows
    img2 += x[3] * rows ** 2
    img2 += x[4] * cols * rows
    img2 += x[5]
    return img2


def numpy_chain(img, ia=None, mask=None, detrend=False):
    """get_n's lines 318-331 in NumPy (the float32 logarithm as the device computes it)."""
    img = img.copy()
    img[img <= 0] = np.nan
    img = 10 * np.log10(img.astype(np.float64)).astype(np.float32)
    if ia is not None:
        img = img - ia * FACTOR
    if mask is not None:
        img[mask] = np.nan
    if detrend:
        img -= numpy_mean(img.shape, lib.fit_spatial_mean(img[::50, ::50]))
    vmin, vmax = np.nanpercentile(img, 10), np.nanpercentile(img, 99)
    u8 = 1 + 254 * (img - vmin) / (vmax - vmin)
    u8[u8 < 1] = 1
    u8[u8 > 255] = 255
    u8[~np.isfinite(img)] = 0
    return u8.astype('uint8')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    import torch
    dev = torch.device('cuda', 0)
    n = args.size
    npix = n * n
    lin, ia, mask = scene(n, dev)
    st = torch.cuda.current_stream().cuda_stream
    work = torch.empty((n, n), dtype=torch.float32, device=dev)
    mean = torch.empty((n, n), dtype=torch.float64, device=dev)
    sub = torch.empty(((n + 49) // 50) ** 2, dtype=torch.float32, device=dev)
    plane = lambda t: (t.data_ptr(), t.stride(0))                                        # noqa: E731
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        coeffs = lib.fit_spatial_mean(lib._prep_subsample(lin, ia, mask, True, FACTOR, torch.cuda.current_stream()))
        _capi.prep_apply(lin.data_ptr(), n, n, n, None, None, True, FACTOR, None, work.data_ptr(), n, st)
        t = {}
        t['a_uint8_ms'] = events_ms(lambda: lib.get_uint8_image(work, None, None, 10, 99), args.reps)
        t['b_db_ms'] = events_ms(lambda: lib.prepare_image(lin), args.reps)
        t['c_full_ms'] = events_ms(lambda: lib.prepare_image(lin, incidence_angle=ia, mask=mask, remove_spatial_mean=True), args.reps)
        t['c_full_given_coeffs_ms'] = events_ms(lambda: lib.prepare_image(lin, incidence_angle=ia, mask=mask, remove_spatial_mean=True,
                                                                          spatial_mean_coeffs=coeffs), args.reps)
        t['apply_db_ms'] = events_ms(lambda: _capi.prep_apply(lin.data_ptr(), n, n, n, None, None, True, FACTOR, None, work.data_ptr(), n, st), args.reps)
        t['apply_copy_ms'] = events_ms(lambda: _capi.prep_apply(lin.data_ptr(), n, n, n, None, None, False, FACTOR, None, work.data_ptr(), n, st), args.reps)
        t['apply_full_ms'] = events_ms(lambda: _capi.prep_apply(lin.data_ptr(), n, n, n, plane(ia), plane(mask), True, FACTOR, coeffs,
                                                                work.data_ptr(), n, st), args.reps)
        t['apply_full_no_db_ms'] = events_ms(lambda: _capi.prep_apply(lin.data_ptr(), n, n, n, plane(ia), plane(mask), False, FACTOR, coeffs,
                                                                      work.data_ptr(), n, st), args.reps)
        t['subsample_ms'] = events_ms(lambda: _capi.prep_subsample(lin.data_ptr(), n, n, n, plane(ia), plane(mask), True, FACTOR, 50,
                                                                   sub.data_ptr(), st), args.reps)
        t['spatial_mean_ms'] = events_ms(lambda: _capi.prep_spatial_mean(n, n, coeffs, mean.data_ptr(), n, st), args.reps)
        t['torch_copy_ms'] = events_ms(lambda: work.copy_(lin), args.reps)
    bytes_moved = dict(apply_db=8 * npix, apply_copy=8 * npix, apply_full=13 * npix, apply_full_no_db=13 * npix, spatial_mean=8 * npix,
                       torch_copy=8 * npix)
    res = dict(device=torch.cuda.get_device_name(0), size=n, reps=args.reps, copy_rate_TBps=COPY_RATE / 1e12)
    res.update({k: round(v, 4) for k, v in t.items()})
    for k, b in bytes_moved.items():
        bound = b / COPY_RATE * 1e3
        res['bytes_' + k] = int(b)
        res['bound_%s_ms' % k] = round(bound, 4)
        res['fraction_of_copy_rate_' + k] = round(bound / t[k + '_ms'], 3)
    for k, b in (('b_db', 8 * npix), ('c_full', 13 * npix)):
        bound = t['a_uint8_ms'] + b / COPY_RATE * 1e3
        res['bound_%s_ms' % k] = round(bound, 4)
        res['ratio_%s_to_bound' % k] = round(t[k + '_ms'] / bound, 3)
    if not args.no_host:
        h_lin, h_ia, h_mask = lin.cpu().numpy(), ia.cpu().numpy(), mask.cpu().numpy()
        with np.errstate(all='ignore'), warnings.catch_warnings():
            warnings.simplefilter('ignore')
            t0 = time.perf_counter()
            exp_b = numpy_chain(h_lin)
            t1 = time.perf_counter()
            exp_c = numpy_chain(h_lin, h_ia, h_mask, True)
            t2 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            got_b = lib.prepare_image(lin).cpu().numpy()
            got_c = lib.prepare_image(lin, incidence_angle=ia, mask=mask, remove_spatial_mean=True).cpu().numpy()
        res.update(host_numpy_b_db_s=round(t1 - t0, 2), host_numpy_c_full_s=round(t2 - t1, 2),
                   host_cpus=len(os.sched_getaffinity(0)), host_threads_env=os.environ.get('OMP_NUM_THREADS'),
                   pixels_differing_b=int((got_b != exp_b).sum()), pixels_differing_c=int((got_c != exp_c).sum()))
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
