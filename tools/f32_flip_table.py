#!/usr/bin/env python3
"""Print what the stand-in of tests/f32_flips.py shows on every frame of its tables (CPU only: the fp64 restatement on a scene whose
shape coefficients are scaled by 1 + 6e-7 u, jitter seeds 5, 6, 7): per frame and seed the pixels moved beyond PIXEL_TOL, the least of
them in units of the pixel's own value, the gradient error before and after the gradient-image correction, and the verdict of the
rule (stable / chaotic).  The numbers behind STRICT_FRAMES and CHAOTIC_FRAMES; profiles/r22_f32_general_form.txt keeps a copy."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import f32_flips as ff  # noqa: E402

pkg = entry.load_package()
oracle = entry.load_oracle()
oracle.lib()


def moved(scene, cam, rp, seed):
    """(pixels the stand-in moves beyond PIXEL_TOL of the largest value, the least of them over the pixel's own value)"""
    ref = oracle.render(scene, cam, rp)["image"]
    img = ff.StandIn(oracle, scene, seed).render(cam, rp)[0].astype(np.float64)
    d = np.abs(img - ref).max(-1)
    bad = d > ff.PIXEL_TOL * np.abs(ref).max()
    own = np.maximum(np.abs(ref).max(-1), np.abs(img).max(-1))
    return int(bad.sum()), (float((d[bad] / own[bad]).min()) if bad.any() else None)


print(f"{'table':8s} {'frame':40s} {'rule':8s} " + " | ".join(f"seed {s}: px  min d/own  before    after   " for s in ff.STANDIN_SEEDS))
for table, frames in (("strict", ff.STRICT_FRAMES), ("chaotic", ff.CHAOTIC_FRAMES)):
    for frame in frames:
        scene, cam, rp, adjoint = ff.frame_inputs(pkg, frame)
        ok, _ = ff.stable(oracle, scene, cam, rp, adjoint, frame[6])
        cells = []
        for seed, rec in zip(ff.STANDIN_SEEDS, ff.standin_records(oracle, scene, cam, rp, adjoint, frame[6])):
            n, r = moved(scene, cam, rp, seed)
            after = ("fails: rounding-sized pixel" if "rounding-sized" in str(rec) else "fails the check") if isinstance(rec, AssertionError) \
                else f"{rec['grad_err']:.2e} {rec['grad_err_corrected']:.2e}"
            cells.append(f"{n:10d}  {'-' if r is None else format(r, '.4f'):>9s}  {after:27s}")
        print(f"{table:8s} {ff.frame_id(frame):40s} {'stable' if ok else 'chaotic':8s} " + " | ".join(cells), flush=True)
print("\nunbiased operator (no gradient image: pixels moved, gradient moved; worst of the three seeds)")
for table, frames in (("strict", ff.UNBIASED_STRICT + [ff.P5_LIKE]), ("chaotic", ff.UNBIASED_CHAOTIC)):
    for frame in frames:
        scene, cam, rp, adjoint = ff.frame_inputs(pkg, frame)
        px, move = ff.unbiased_move(oracle, scene, cam, rp, adjoint)
        print(f"{table:8s} {ff.frame_id(frame) + (f' seed {rp.seed}' if frame is ff.P5_LIKE else ''):40s} {px:3d} px  {move:.2e}")
