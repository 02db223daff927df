#!/usr/bin/env python3
"""Timings of the area-average downsampling (sea_ice_drift_amd.lib.resize_image, include/sid_resize.h) and of the fused front of
prepare_image_resized(factor=) on a 10000 x 10000 float32 scene: device tensors in and out, HIP events on the stream, every row warmed
up, then --reps rounds in which the rows take turns, median and spread (min, max) per row.  The rows named kernel_* and pass_*
call the C ABI on buffers allocated once, five calls back to back between the two events (the time is a fifth of it), so
that the device and not the host's enqueue is what is timed; the others are one call of the public function, allocation of
the result and Python included.

  kernel_f32_0.5 / _0.25 / _0.4   sid_resize_f32 of the float32 scene (0.4 is a fractional ratio: 5 source pixels per 2 outputs)
  kernel_u8_0.5                   sid_resize_u8 of a uint8 scene
  kernel_avg_pool2d_0.5           torch.nn.functional.avg_pool2d(x[None, None], 2) on the same tensor, five calls: the yardstick
  resize_f32_* / resize_u8_0.5 / avg_pool2d_0.5      one call of lib.resize_image / of avg_pool2d
  pass_fused_* / pass_two_*       the float32 working image of prepare_image_resized(factor=0.5): sid_resize_prep_apply, against
                                  sid_resize_f32 of the planes + sid_prep_apply (db: dB only; full: dB + HH + detrend with given
                                  coefficients)
  prepare_fused_* / prepare_two_* the whole prepare_image (percentiles and uint8 staging included) both ways, one call
  bytes_*, bound_*_ms             bytes the pass has to move and that over 6.29 TB/s (the measured float4 copy rate)
  ratio_*                         measured / bound
  parity_*                        pixels that differ from the specification (tests/resize_spec.py) on the crop stated in `parity_crop`,
                                  and of the fused results from the two-call ones on the whole scene
  host_numpy_block_mean_s         x.reshape(n/2, 2, n/2, 2).mean((1, 3), dtype=float64) on this host (one run; --no-host skips it)

    python tools/resize_bench.py [--size 10000] [--reps 20] [--out FILE] [--no-host]
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
from tests import resize_spec as spec                      # noqa: E402

COPY_RATE = 6.29e12                                        # bytes / s, float4 copy on the MI355X
HH_FACTOR = -0.27
COEFFS = np.array([-1.1e-3, 4.0e-8, 2.0e-5, -1.0e-9, 3.0e-9, -21.5])
CROP_ROWS = 1000
INNER = 5                                                  # calls between two events in the kernel_* and pass_* rows


def scene(n, device):
    import torch
    g = torch.Generator(device=device).manual_seed(7)
    c = torch.arange(n, device=device, dtype=torch.float32)[None, :]
    db = -18.0 - 9.0 * c / n + 4.0 * torch.randn((n, n), device=device, generator=g)
    lin = torch.pow(10.0, db / 10.0)
    u = torch.rand((n, n), device=device, generator=g)
    lin[u < 0.002] = float('nan')
    lin[(u >= 0.002) & (u < 0.004)] = 0.0
    lin[:, :30] = 0.0
    ia = (20.0 + 26.0 * c / n).expand(n, n).contiguous()
    u8 = (torch.rand((n, n), device=device, generator=g) * 255.99).to(torch.uint8)
    del db, u
    return lin, ia, u8


def take_turns(rows, reps, warmup=3):
    """{name: (median, min, max) in ms per call}: every row (name -> (function, calls between the events)) warmed up, then
    `reps` rounds in which the rows take turns."""
    import torch
    for fn, _ in rows.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in rows}
    for _ in range(reps):
        for k, (fn, inner) in rows.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            ts[k].append(a.elapsed_time(b) / inner)
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in ts.items()}


def differing(a, b):
    """Pixels of two host arrays that differ (every NaN the same value)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == 'f':
        return int((~((a == b) & (np.signbit(a) == np.signbit(b)) | (np.isnan(a) & np.isnan(b)))).sum())
    return int((a != b).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=10000)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F
    if not torch.cuda.is_available():
        raise SystemExit('resize_bench measures on the GPU: no device is visible')
    dev = torch.device('cuda', 0)
    n = args.size
    lin, ia, u8 = scene(n, dev)
    half = lib.resize_shape(n, n, 0.5)

    def work(img, ang, coeffs, factor):
        return lib._prep_apply(img, ang, None, True, HH_FACTOR, coeffs is not None, coeffs, 0, factor)[0]

    def two_pass(ang, coeffs):
        return work(lib.resize_image(lin, 0.5), None if ang is None else lib.resize_image(ang, 0.5), coeffs, 1)

    def two_prepare(ang, coeffs):
        return lib.prepare_image(lib.resize_image(lin, 0.5), incidence_angle=None if ang is None else lib.resize_image(ang, 0.5),
                                 remove_spatial_mean=coeffs is not None, spatial_mean_coeffs=coeffs)

    st = torch.cuda.current_stream().cuda_stream
    plane = lambda x: (x.data_ptr(), x.stride(0))                                        # noqa: E731
    outs = {f: torch.empty(lib.resize_shape(n, n, f), dtype=torch.float32, device=dev) for f in (0.5, 0.25, 0.4)}
    out_u8 = torch.empty(half, dtype=torch.uint8, device=dev)
    small, small_ia, out_work = [torch.empty(half, dtype=torch.float32, device=dev) for _ in range(3)]

    def k_resize(src, dtype, dst, option=False):
        _capi.resize(src.data_ptr(), dtype, n, n, src.stride(0), dst.data_ptr(), dst.shape[0], dst.shape[1], dst.stride(0), option, st)

    def k_fused(ang, coeffs):
        _capi.resize_prep_apply(lin.data_ptr(), n, n, n, None if ang is None else plane(ang), None, True, HH_FACTOR, coeffs,
                                out_work.data_ptr(), half[0], half[1], half[1], st)

    def k_two(ang, coeffs):
        k_resize(lin, 'float32', small)
        if ang is not None:
            k_resize(ang, 'float32', small_ia)
        _capi.prep_apply(small.data_ptr(), half[0], half[1], half[1], None if ang is None else plane(small_ia), None, True, HH_FACTOR,
                         coeffs, out_work.data_ptr(), half[1], st)

    rows = {
        'kernel_f32_0.5': (lambda: k_resize(lin, 'float32', outs[0.5]), INNER),
        'kernel_avg_pool2d_0.5': (lambda: F.avg_pool2d(lin[None, None], 2), INNER),
        'kernel_f32_0.25': (lambda: k_resize(lin, 'float32', outs[0.25]), INNER),
        'kernel_f32_0.4': (lambda: k_resize(lin, 'float32', outs[0.4]), INNER),
        'kernel_u8_0.5': (lambda: k_resize(u8, 'uint8', out_u8, True), INNER),
        'pass_fused_db': (lambda: k_fused(None, None), INNER),
        'pass_two_db': (lambda: k_two(None, None), INNER),
        'pass_fused_full': (lambda: k_fused(ia, COEFFS), INNER),
        'pass_two_full': (lambda: k_two(ia, COEFFS), INNER),
        'resize_f32_0.5': (lambda: lib.resize_image(lin, 0.5), 1),
        'avg_pool2d_0.5': (lambda: F.avg_pool2d(lin[None, None], 2), 1),
        'resize_f32_0.25': (lambda: lib.resize_image(lin, 0.25), 1),
        'resize_f32_0.4': (lambda: lib.resize_image(lin, 0.4), 1),
        'resize_u8_0.5': (lambda: lib.resize_image(u8, 0.5), 1),
        'prepare_fused_db': (lambda: lib.prepare_image_resized(lin, factor=0.5), 1),
        'prepare_two_db': (lambda: two_prepare(None, None), 1),
        'prepare_fused_full': (lambda: lib.prepare_image_resized(lin, incidence_angle=ia, remove_spatial_mean=True, spatial_mean_coeffs=COEFFS,
                                                                 factor=0.5), 1),
        'prepare_two_full': (lambda: two_prepare(ia, COEFFS), 1),
    }
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        t = take_turns(rows, args.reps)
    npix = n * n
    out_pix = {f: int(np.prod(lib.resize_shape(n, n, f))) for f in (0.5, 0.25, 0.4)}
    bytes_moved = {
        'kernel_f32_0.5': 4 * npix + 4 * out_pix[0.5], 'kernel_avg_pool2d_0.5': 4 * npix + 4 * out_pix[0.5],
        'kernel_f32_0.25': 4 * npix + 4 * out_pix[0.25], 'kernel_f32_0.4': 4 * npix + 4 * out_pix[0.4],
        'kernel_u8_0.5': npix + out_pix[0.5],
        'pass_fused_db': 4 * npix + 4 * out_pix[0.5], 'pass_fused_full': 8 * npix + 4 * out_pix[0.5],
        # two calls: the reduced planes are written and read back
        'pass_two_db': 4 * npix + 4 * out_pix[0.5] + 8 * out_pix[0.5], 'pass_two_full': 8 * npix + 8 * out_pix[0.5] + 12 * out_pix[0.5],
    }
    res = dict(device=torch.cuda.get_device_name(0), size=n, reps=args.reps, calls_per_timing=INNER, copy_rate_TBps=COPY_RATE / 1e12, half_shape=list(half))
    for k, (med, lo, hi) in t.items():
        res[k + '_ms'] = round(med, 4)
        res[k + '_min_ms'] = round(lo, 4)
        res[k + '_max_ms'] = round(hi, 4)
    for k, b in bytes_moved.items():
        bound = b / COPY_RATE * 1e3
        res['bytes_' + k] = int(b)
        res['bound_%s_ms' % k] = round(bound, 4)
        res['ratio_' + k] = round(t[k][0] / bound, 3)
    # parity with the specification on the first CROP_ROWS rows (a multiple of every window height here: 2, 4, 5), all columns
    crop = min(CROP_ROWS, n - n % 20)
    res['parity_crop'] = '[0:%d, 0:%d] of the scene' % (crop, n)
    h_lin, h_u8 = lin[:crop].cpu().numpy(), u8[:crop].cpu().numpy()
    for f in (0.5, 0.25, 0.4):
        shape = lib.resize_shape(crop, n, f)
        got = lib.resize_image(lin[:crop], f).cpu().numpy()
        res['parity_resize_f32_%s' % f] = differing(got, spec.resize_f32(h_lin, *shape))
        full = lib.resize_image(lin, f)[:shape[0]].cpu().numpy()
        res['parity_resize_f32_%s_full_vs_crop' % f] = differing(full[:, :shape[1]], got) if full.shape[1] == shape[1] else -1
    shape = lib.resize_shape(crop, n, 0.5)
    res['parity_resize_u8_0.5'] = differing(lib.resize_image(u8[:crop], 0.5).cpu().numpy(), spec.resize_u8(h_u8, *shape))
    res['avg_pool2d_differs_from_resize'] = differing(F.avg_pool2d(lin[None, None], 2)[0, 0].cpu().numpy(), lib.resize_image(lin, 0.5).cpu().numpy())
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        for tag, ang, coeffs in (('db', None, None), ('full', ia, COEFFS)):
            res['parity_pass_fused_vs_two_' + tag] = differing(work(lin, ang, coeffs, 0.5).cpu().numpy(), two_pass(ang, coeffs).cpu().numpy())
            fused = lib.prepare_image_resized(lin, incidence_angle=ang, remove_spatial_mean=coeffs is not None, spatial_mean_coeffs=coeffs, factor=0.5)
            res['parity_prepare_fused_vs_two_' + tag] = differing(fused.cpu().numpy(), two_prepare(ang, coeffs).cpu().numpy())
    if not args.no_host and n % 2 == 0:
        h = lin.cpu().numpy()
        t0 = time.perf_counter()
        block = h.reshape(n // 2, 2, n // 2, 2).mean((1, 3), dtype=np.float64)
        res['host_numpy_block_mean_s'] = round(time.perf_counter() - t0, 3)
        res['host_cpus'] = len(os.sched_getaffinity(0))
        del block
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
