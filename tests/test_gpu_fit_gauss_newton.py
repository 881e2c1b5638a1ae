"""tools/fit_albedo.py --gauss-newton on the device: the red wall's albedo (0.5, 0, 0) recovered from (0.2, 0.2, 0.2) by Levenberg-Marquardt
steps on drt_hip_render_normal_equations, at the tool's defaults (128 x 128, 16 spp, depth 8), to the bound the tool's main() exits 0 on
(max error <= 1e-2).

N = 5: the CPU loop (`--gauss-newton --oracle`, the same frame size, the restatement in fp64) is within the bound after its fifth step
(max errors after steps 2 to 7: 0.053, 0.023, 0.016, 0.0089, 0.0088, 0.0049; HISTORY.md has the trace).  The device gets N + 2 = 7 steps for
f32 and seed differences -- against the 60 steps of the Adam route (tests/test_gpu_fit.py).  At 16 spp a single step's estimate scatters by
~0.006 around the solution (the noise of b = J^T r), which is what the bound leaves room for.
The target's zero channels are reached from 0.2: the steps drive a colour INTO a zero channel (k_path's zc bookkeeping in the Jacobian form)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))

N = 5


def test_gauss_newton_recovers_the_albedo(pkg):
    import fit_albedo
    assert fit_albedo.GN_STEPS == N
    size, spp, steps = 128, 16, N + 2
    render = fit_albedo.DeviceRender(pkg, size, spp, 8)
    try:
        rgb, hist = fit_albedo.fit_gauss_newton(render, 0, np.array([0.2, 0.2, 0.2]), steps, log=print)
    finally:
        render.r.close()
    assert steps < 60
    assert np.abs(rgb - np.array([0.5, 0.0, 0.0])).max() <= 1e-2, rgb
    assert rgb[1] <= 1e-2 and rgb[2] <= 1e-2 and hist[0][1] < 0.2 and hist[0][2] < 0.2     # the zero channels, from above
    assert render.calls == 4 * steps
