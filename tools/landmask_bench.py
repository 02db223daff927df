#!/usr/bin/env python3
"""Timings of the invalid-pixel mask (sea_ice_drift_amd.lib.invalid_mask, include/sid_mask.h) for a 500 x 500 water mask zoomed to a
10000 x 10000 float32 scene, device tensors in and out, HIP events on the stream, median of --reps calls after warm-up:

  invalid_mask_ms          lib.invalid_mask(img, wm): filter, prefilter and the full-resolution pass, the output plane allocated per call
  mask_invalid_capi_ms     sid_mask_invalid alone into a plane that exists (the same three steps)
  nonfinite_capi_ms        sid_mask_invalid without a water mask (isnan | isinf: 4 B in, 1 B out per pixel)
  landmask_capi_ms         sid_mask_landmask (no image: 1 B out per pixel)
  prep_apply_db_ms         the dB-only pass of sid_prep_apply on the same scene (4 B in, 4 B out per pixel): the yardstick
  ratio_to_prep_apply_db   mask_invalid_capi_ms / prep_apply_db_ms
  prepare_mask_invalid_ms  lib.prepare_image_masked(img, mask_invalid=True, watermask=wm); prepare_plain_ms: lib.prepare_image(img)
  bytes_* / GBps_*         bytes the algorithm moves (computed from the shapes) and the rate they were moved at
  scipy_zoom_s             maximum_filter + zoom of the same raster with SciPy on this host (one run), scipy_mask_s the whole
                           reference get_invalid_mask arithmetic; mask_bytes_differing / wmz_bytes_differing: full-plane comparison
                           of the device's results with SciPy's, outside the timed region (--no-host skips these)
Kernel times alone: run under `rocprofv3 --kernel-trace --stats` (kernels zoom_mask_kernel<...>, clip_max3_kernel,
lw_spline_pass_kernel<...>).

    python tools/landmask_bench.py [--size 10000] [--border 20] [--reps 20] [--out FILE] [--no-host]
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


def scene(n, device):
    import torch
    g = torch.Generator(device=device).manual_seed(7)
    c = torch.arange(n, device=device, dtype=torch.float32)[None, :]
    lin = torch.pow(10.0, (-18.0 - 9.0 * c / n + 4.0 * torch.randn((n, n), device=device, generator=g)) / 10.0)
    u = torch.rand((n, n), device=device, generator=g)
    lin[u < 0.02] = float('nan')
    lin[(u >= 0.02) & (u < 0.025)] = float('inf')
    lin[(u >= 0.025) & (u < 0.03)] = float('-inf')
    del u
    return lin


def raster(m):
    """A coast: land (2) where a smooth random field is high, a fringe of 1, open water 0, a few codes above 2."""
    rng = np.random.default_rng(11)
    f = rng.standard_normal((m // 10 + 2, m // 10 + 2))
    from scipy.ndimage import zoom
    f = zoom(f, 10, order=3)[:m, :m]
    wm = np.zeros((m, m), dtype=np.uint8)
    wm[f > 0.3] = 1
    wm[f > 0.5] = 2
    wm[rng.random((m, m)) > 0.995] = 7
    return wm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=10000)
    ap.add_argument('--border', type=int, default=20)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--no-host', action='store_true')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('landmask_bench: no GPU (nothing is measured without one)')
    dev = torch.device('cuda', 0)
    n, m = args.size, args.size // args.border
    npix = n * n
    lin = scene(n, dev)
    h_wm = raster(m)
    wm = torch.from_numpy(h_wm).to(dev)
    st = torch.cuda.current_stream().cuda_stream
    plane = lambda t: (t.data_ptr(), t.stride(0))                                        # noqa: E731
    out = torch.empty((n, n), dtype=torch.uint8, device=dev)
    wmz = torch.empty((n, n), dtype=torch.uint8, device=dev)
    work32 = torch.empty((n, n), dtype=torch.float32, device=dev)
    ws = torch.empty(_capi.mask_workspace_bytes(m, m), dtype=torch.uint8, device=dev)
    t = {}
    with contextlib.redirect_stdout(io.StringIO()), warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        t['invalid_mask_ms'] = events_ms(lambda: lib.invalid_mask(lin, wm), args.reps)
        t['mask_invalid_capi_ms'] = events_ms(lambda: _capi.mask_invalid(plane(wm), m, m, n, n, ws.data_ptr(), plane(lin), False, None, 0.0,
                                                                       plane(out), None, st), args.reps)
        t['nonfinite_capi_ms'] = events_ms(lambda: _capi.mask_invalid(None, 0, 0, n, n, 0, plane(lin), False, None, 0.0, plane(out), None, st),
                                           args.reps)
        t['landmask_capi_ms'] = events_ms(lambda: _capi.mask_landmask(plane(wm), m, m, n, n, ws.data_ptr(), plane(out), None, st), args.reps)
        t['prep_apply_db_ms'] = events_ms(lambda: _capi.prep_apply(lin.data_ptr(), n, n, n, None, None, True, -0.27, None, work32.data_ptr(), n, st),
                                          args.reps)
        t['prepare_mask_invalid_ms'] = events_ms(lambda: lib.prepare_image_masked(lin, mask_invalid=True, watermask=wm), args.reps)
        t['prepare_plain_ms'] = events_ms(lambda: lib.prepare_image(lin), args.reps)
    res = dict(device=torch.cuda.get_device_name(0), size=n, watermask=m, reps=args.reps)
    res.update({k: round(v, 4) for k, v in t.items()})
    res['ratio_to_prep_apply_db'] = round(t['mask_invalid_capi_ms'] / t['prep_apply_db_ms'], 3)
    small = m * m * (1 + 1 + 8 * 16)                       # raster read, filtered raster, the prefilter's four float64 passes (read + write)
    for k, b in (('mask_invalid_capi', 5 * npix + small), ('nonfinite_capi', 5 * npix), ('landmask_capi', npix + small), ('prep_apply_db', 8 * npix)):
        res['bytes_' + k] = int(b)
        res['GBps_' + k] = round(b / (t[k + '_ms'] * 1e-3) / 1e9, 1)
    if not args.no_host:
        from scipy.ndimage import maximum_filter, zoom
        h_img = lin.cpu().numpy()
        t0 = time.perf_counter()
        mask = np.isnan(h_img) + np.isinf(h_img)
        w2 = h_wm.copy()
        w2[w2 > 2] = 2
        t1 = time.perf_counter()
        z = zoom(maximum_filter(w2, 3), np.array(h_img.shape) / np.array(w2.shape))
        t2 = time.perf_counter()
        mask[z == 2] = True
        t3 = time.perf_counter()
        _capi.mask_invalid(plane(wm), m, m, n, n, ws.data_ptr(), plane(lin), False, None, 0.0, plane(out), plane(wmz), st)
        res.update(scipy_zoom_s=round(t2 - t1, 2), scipy_mask_s=round(t3 - t0, 2), host_cpus=len(os.sched_getaffinity(0)),
                   mask_bytes_differing=int((out.cpu().numpy() != mask.view(np.uint8)).sum()),
                   wmz_bytes_differing=int((wmz.cpu().numpy() != z).sum()),
                   api_mask_bytes_differing=int((lib.invalid_mask(lin, wm).cpu().numpy() != mask).sum()),
                   land_pixels=int((z == 2).sum()), overshoot_pixels=int((z == 3).sum()), nonfinite_pixels=int((~np.isfinite(h_img)).sum()),
                   speedup_over_scipy=round((t3 - t0) / (t['invalid_mask_ms'] * 1e-3), 0))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
