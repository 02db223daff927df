#!/usr/bin/env python3
"""Matcher benchmark: the reference notebook's case (examples/simple.ipynb cell 2: 24 183 x 22 694 ORB
descriptors matched in 3.42 s by cv2.BFMatcher on unknown hardware) on sid_ft_knn2.  Prints one JSON line."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from sea_ice_drift_amd import _capi
from oracle import ft_oracle as fo

n1, n2 = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (24183, 22694)
rng = np.random.default_rng(1)
d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
t0 = time.perf_counter(); idx, dist = _capi.ft_knn2(d1, d2); t_host = time.perf_counter() - t0
t0 = time.perf_counter(); idx, dist = _capi.ft_knn2(d1, d2); t_host = min(t_host, time.perf_counter() - t0)
dev = torch.device('cuda:0')
a, b = torch.from_numpy(d1).to(dev), torch.from_numpy(d2).to(dev)
oi = torch.empty((n1, 2), dtype=torch.int32, device=dev); od = torch.empty_like(oi)
ws = torch.empty(_capi.ft_workspace_bytes(n1, n2), dtype=torch.uint8, device=dev)
st = torch.cuda.current_stream().cuda_stream
def run():
    _capi.ft_knn2_device(a.data_ptr(), n1, b.data_ptr(), n2, oi.data_ptr(), od.data_ptr(), ws.data_ptr(), st)
run(); torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(10): run()
e1.record(); torch.cuda.synchronize()
t_kernel = e0.elapsed_time(e1) / 10 * 1e-3
assert np.array_equal(oi.cpu().numpy(), idx) and np.array_equal(od.cpu().numpy(), dist)
m = min(n1, 2000)
t0 = time.perf_counter(); eidx, edist = fo.knn2(d1[:m], d2); t_cpu = (time.perf_counter() - t0) * n1 / m
ok = bool(np.array_equal(eidx, idx[:m]) and np.array_equal(edist, dist[:m]))
pairs = float(n1) * n2
print(json.dumps({'metric': 'Hamming kNN (k=2) descriptor match', 'n1': n1, 'n2': n2,
                  'kernel_ms': t_kernel * 1e3, 'pairs_per_s': pairs / t_kernel,
                  'form': 'mfma (256 int8 MACs + 4 VALU lane-ops per pair)' if _capi.ft_debug_plan(n1, n2)['mfma']
                          else 'one thread per query (21 VALU lane-ops per pair: 8 xor + 8 bcnt + key + 3 min/max)',
                  'host_call_ms_incl_alloc_and_pcie': t_host * 1e3,
                  'numpy_oracle_s_extrapolated_from_%d_queries' % m: t_cpu, 'parity_vs_oracle_sample': ok,
                  'reference_notebook_s': 3.42 if (n1, n2) == (24183, 22694) else None}))
