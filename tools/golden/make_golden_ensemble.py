"""Golden for the ensemble / MC-dropout mutual-information baselines: run the REFERENCE's ComputeMI (mmdet/apis/CalEnsembleUnc.py) and
ComputeMCDropoutMI (mmdet/apis/CalMCDropoutUnc.py) on seeded logit maps and record inputs + outputs in tests/golden/ensemble_mi.npz.

    python tools/golden/make_golden_ensemble.py

Cases (B = 3, levels (4, 6), (2, 3), (1, 2), A * C = 2 * 20):
    prior_k3      K = 3 through ComputeMI,          logits ~ N(-4.6, 2^2): the focal-loss prior region
    prior_k5      K = 5 through ComputeMCDropoutMI, same distribution
    saturated_k3  K = 3 through ComputeMI,          logits uniform in +-30 (saturated sigmoids, still finite in the reference)
The logits are rounded to multiples of 2^-10 (exact in fp32), which keeps the compressed fixture under its size limit.
Per case: {case}_x{l} [K, B, 40, h, w] float32, {case}_ref [B] (the reference's output), {case}_e_ref (max |ref - float64 restatement|),
{case}_total_mean (float64 mean of the `total` term)."""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
warnings.filterwarnings('ignore')
import mmcv_shim  # noqa: E402

mmcv_shim.install()
try:
    import cv2  # noqa: F401
except Exception:      # noqa: BLE001
    sys.modules['cv2'] = types.ModuleType('cv2')
from mmdet.apis.CalEnsembleUnc import ComputeMI  # noqa: E402
from mmdet.apis.CalMCDropoutUnc import ComputeMCDropoutMI  # noqa: E402

from tests.ensemble_mi_util import CASES, LEVELS, mi_float64  # noqa: E402

B, AC, NCLS = 3, 40, 20


def logits(seed, K, saturated):
    g = torch.Generator().manual_seed(seed)
    xs = []
    for h, w in LEVELS:
        if saturated:
            x = (torch.rand(K, B, AC, h, w, generator=g) * 2 - 1) * 30
        else:
            x = torch.randn(K, B, AC, h, w, generator=g) * 2 - 4.6
        xs.append(torch.round(x * 1024) / 1024)
    return xs


out = {}
for name, seed, K, fn, sat in ((CASES[0], 4101, 3, ComputeMI, False), (CASES[1], 4102, 5, ComputeMCDropoutMI, False),
                               (CASES[2], 4103, 3, ComputeMI, True)):
    xs = logits(seed, K, sat)
    members = [[x[k] for x in xs] for k in range(K)]             # member -> levels -> [B, A*C, h, w]
    with torch.no_grad():
        ref = np.asarray(fn(*members, nCls=NCLS), np.float64)
    assert ref.shape == (B,) and np.isfinite(ref).all(), (name, ref)
    f64, total_mean = mi_float64([[t.numpy() for t in m] for m in members], NCLS)
    for l, x in enumerate(xs):
        out[f'{name}_x{l}'] = x.numpy().astype(np.float32)
    out[f'{name}_ref'] = ref.astype(np.float32)
    out[f'{name}_e_ref'] = np.float64(np.abs(ref - f64).max())
    out[f'{name}_total_mean'] = np.float64(total_mean)
    print(name, 'ref', ref, 'e_ref', out[f'{name}_e_ref'], 'total_mean', total_mean)
path = os.path.join(ROOT, 'tests', 'golden', 'ensemble_mi.npz')
np.savez_compressed(path, **out)
size = os.path.getsize(path)
print('ensemble_mi golden:', size, 'bytes')
assert size <= 150 * 1024, size
