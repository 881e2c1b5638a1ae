#!/usr/bin/env python3
"""An inverse-rendering loop over the path (the use the reference is written for, /root/reference/README.md:88-101:
render -> loss -> backward -> parameter step), on the device through the C ABI:

    target  = render(scene with red = (0.5, 0, 0))                               once, 256 spp
    repeat:   image = drt_hip_render(seed A)                                     forward only
              adjoint = d loss / d pixel = 2 (image - target) / N                loss = mean squared error over the N pixel values
              gradient = drt_hip_render(seed B, BACKWARD, adjoint_rgb) / spp     out_param_grad is the SUM over the samples
              Adam step on the red albedo, clip to [0, 1], drt_hip_update_params

The image the adjoint comes from and the samples the gradient is taken on are INDEPENDENT (two seeds per step): with one
sample set for both, E[(I - T) dI] carries the covariance of a pixel's estimate with its own derivative, and the minimum of
the noisy objective sits ~9 % below the true albedo at 16 spp.  The per-pixel adjoint is exact for a loss on the pixel MEANS
(the ABI's adjoint_rgb seeds every sample of a pixel alike); the reference's per-sample `loss_func(radiance).backward()` is
the same thing for a loss that is linear in the radiance.

    python tools/fit_albedo.py [--size 128] [--spp 16] [--steps 60] [--async] [--oracle] [--gauss-newton [--one-render [--cross [--lambda-sets N]]] [--lambda-sets N]]
    python tools/fit_albedo.py --scene cornell_shapes --multi-start N [--oracle]
    python tools/fit_albedo.py --views N [--size 32] [--spp 8] [--steps 60]
    python tools/fit_albedo.py --views N --pixels M [--size 32] [--spp 8] [--steps 60]

--views N (N <= 64): the first loop above against N target views at once, cameras on an arc in front of the box: per step ONE
drt_hip_render_views forward on seed A and ONE backward on seed B with the N adjoint images, whose summed gradient is the gradient of the mean
squared error over all views; the loss is printed per step (fresh seeds: mostly noise at a few samples), and the loss on ONE fixed seed at
128 spp before and after the fit, which decides the exit status.

--async: the same loop through drt_hip_render_async / drt_hip_wait (frame i + 1 needs the parameters of step i, so frames
cannot overlap: what is measured is the call overhead).  --oracle: the CPU restatement instead of the device (checker;
used to choose the optimiser's constants in the build container, which has no GPU).

--gauss-newton: the second-order route over the same two-seed loop, drt_hip_render_normal_equations instead of the backward render:

    repeat:   image = drt_hip_render(seed A)                  r = image - target
              A, b  = drt_hip_render_normal_equations(seed B, residual_rgb = r)       J^T J and J^T r per channel, from one render,
                                                                                     and that render's own image: r' = image_B - target
              step  = -(A + lambda diag A)^-1 b  on the red albedo (a 1 x 1 system per channel: colour channels do not mix)
              candidate = clip(red + step, 0, 1), rendered with seed A and with seed B
              loss = sum r r' here and at the candidate;  smaller there: accept, lambda / 3;  else keep red, lambda x 4

The loss that decides is the product of TWO independent residuals, for the reason the gradient takes two seeds: sum r^2 of one sample
set holds the variance of every pixel's estimate, which grows with the albedo, and rejects steps towards the true value (at 48 x 48 x
16 spp the one-set loss rises along the whole correct step).  Both losses use the same two sample sets, so they differ by the step and
not by their noise.  Levenberg-Marquardt with the usual accept / reject update of lambda: four renders per step, --steps of them
(default here: GN_STEPS).
--one-render: target_rgb instead of residual_rgb, ONE seed and ONE render per step (every step is accepted, lambda stays): r and J then
share their samples, b = J^T r carries the covariance of a pixel's estimate with its own derivative, and the fit settles where the noisy
objective has its minimum -- ~9 % below the true albedo at 16 spp with one sample set for the first-order loop (the figure above).
Here the same covariance is divided by a J^T J that the pixels' variance inflates, and the Gauss-Newton fixed point is lower still:
measured on the device at the defaults, red settles at 0.286 (6 steps, the last two 0.2866 and 0.2857), so this form exits with
status 1 at the defaults; it is for frames with enough samples that the bias is below what the caller needs.
--one-render --cross: the one-render loop on drt_hip_render_normal_equations_cross (the device only).  b and the loss are then the means
over ordered pairs of DIFFERENT samples of each pixel -- unbiased from the one render: the covariance and the variance above are
subtracted, estimated from the same samples --, so the loss can decide again.  One call per step, on a fresh seed: it gives the
candidate's loss, compared with the current point's (from the call that produced the step: smaller: accept, lambda / 3; else keep,
lambda x 4), and, where the candidate is accepted, the next step.  --steps + 1 renders.  Measured on the device at the defaults: the
first step is accepted (red 0.3677, loss 0.590 with a subtracted noise floor of 14.48) and the four candidates after it are rejected,
so red stays at 0.3677 and this form exits with status 1 too: the two losses that are compared come from different sample sets, and
what is left of the loss after the subtraction is 1 / 25 of the noise floor.  The values are unbiased (tests/test_gpu_cross.py); a
loop that compares them across seeds at 16 spp is not yet a fit.
--one-render --cross --lambda-sets N (N <= 7): the comparison on COMMON paths.  Per step one drt_hip_render_normal_equations_cross call at
the current point (seed A: the step for each of N dampings), then ONE drt_hip_render_param_sets_cross call on a fresh seed B that prices
[current, candidate_1 ... candidate_N] on the same paths, each loss unbiased: the best candidate is accepted iff its loss~ is below the
current point's on that trace (lambda becomes the winner's / 3; else the largest tried x 4).  Two traces per step.  Measured on the device at the defaults with N = 3: four steps accepted (red 0.3678, 0.4421, 0.4800, 0.4878), the
fifth rejected (loss~ 0.903306 at the current point against 0.903329 for the best candidate on the same trace): fitted red (0.4878, 0.0118,
0.0139) in 10 renders, 0.0139 from the truth -- status 1 against this tool's bound of 1e-2, beside 0.3677, 0.2866 and the two-seed loop's
0.4960 in 20 renders.
--oracle runs the same loop on the CPU restatement, J assembled from oracle.render(backward=True, grad_image_param=p).
--lambda-sets N (N <= 7): after the two normal-equation renders the candidates for lambda x {1, 1/3, 4, 1/9, 16, 1/27, 64}[:N] are
evaluated in ONE drt_hip_render_param_sets call per seed (one trace for all N: a parameter does not decide where a path goes), the
smallest two-seed loss sum r_A r_B wins and is accepted if it is below the current one (lambda becomes the winner's / 3; else the
largest tried x 4).  A step is still four renders, of which two are traces of N candidates.

--line-search N (N <= 4, with --scene cornell_shapes): the block's Gauss-Newton direction delta (the step of the current lambda) is kept and its
LENGTH is searched: the N step lengths alpha x {1, 1/2, 2, 1/4}[:N] are evaluated as params + alpha delta with direction delta in ONE
drt_hip_render_param_sets_along call per seed -- images and their derivatives along delta from one trace --, which gives per step length
the two-seed loss phi = sum r_A r_B and its slope phi' = sum (t_A r_B + r_A t_B).  Where two neighbouring step lengths bracket a minimum
(phi' < 0 then phi' > 0) the step is the minimiser of the cubic through both (phi, phi') pairs; else the best candidate, accepted if it is
below the current loss.  A step is still four renders per block, of which two are traces of N candidates.

--gauss-newton --scene cornell_shapes: ALL parameters of a scene past the eight the normal equations take (ten: an albedo per shape, the
unused `white`, the emission), from a perturbed start, through drt_hip_render_normal_equations_along -- unit-vector directions in blocks
of at most eight (8 + 2), block Gauss-Seidel: per step every block in turn takes the two-seed Levenberg-Marquardt step above (its own
K x K system per channel; a row whose diagonal is zero -- `white`, a channel nothing depends on -- stays where it is), 4 renders per
block.  --subspace tint fits ONE tint over the albedos instead (three directions d theta / d tint_ch, one block).  Printed beside it:
Adam over the same parameters from the same start with the same number of renders, and both fits' loss on a fixed pair of evaluation
seeds (sum of r_A r_B, the unbiased estimate of the squared error against the target).

--multi-start N (N <= 8, with --scene): N perturbed starts run as N Adam chains over every parameter, side by side.  Per step ONE
drt_hip_render_param_sets call (seed A: the N images the adjoints 2 (image_k - target) / n come from) and ONE
drt_hip_render_param_sets_grad call (seed B: the N gradients, each chain seeded with its own adjoint) -- two traces per step where N
separate runs of the first-order loop need 2 N.  Printed: every chain's two-seed loss at its start and at its end, and the best.
--oracle runs the same chains as a loop over the restatement."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def fit(render, n_params, p_index, start, steps, spp, n_values, lr=0.08, decay=0.96, log=None):
    """render(params [P,3], seed, backward, adjoint) -> (image [H,W,3], grads [P,3] | None).  Adam on parameter p_index.
    -> (fitted rgb, history of rgb per step)"""
    params = render.params0.copy()
    params[p_index] = start
    m = np.zeros(3); v = np.zeros(3)
    b1, b2, eps = 0.8, 0.99, 1e-8
    hist = []
    for k in range(steps):
        img, _ = render(params, 1000 + 2 * k, False, None)
        adj = (2.0 * (img.astype(np.float64) - render.target) / n_values).astype(np.float32)
        _, grads = render(params, 1001 + 2 * k, True, adj)
        g = grads[p_index] / spp
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        step = lr * decay ** k * (m / (1 - b1 ** (k + 1))) / (np.sqrt(v / (1 - b2 ** (k + 1))) + eps)
        params[p_index] = np.clip(params[p_index] - step, 0.0, 1.0)
        hist.append(params[p_index].copy())
        if log:
            loss = float(((img.astype(np.float64) - render.target) ** 2).mean())
            log(f"step {k:3d}  loss {loss:.6f}  red = ({params[p_index][0]:.4f}, {params[p_index][1]:.4f}, {params[p_index][2]:.4f})")
    return params[p_index].copy(), hist


ALONG_STEPS = 4       # block Gauss-Seidel steps over cornell_shapes by default (64 x 64 x 8: what the CPU loop needs, tests/test_gpu_tangents.py has its trace)
GN_STEPS = 5          # Gauss-Newton steps the tool takes by default: what the CPU loop (--oracle) needs at 128 x 128 x 16 (HISTORY.md has its trace)


LAMBDA_FACTORS = (1.0, 1.0 / 3.0, 4.0, 1.0 / 9.0, 16.0, 1.0 / 27.0, 64.0)


def best_of_lambdas(render, params, lam, n_sets, sa, sb, candidate, lo=0.0, hi=1.0):
    """the candidates params + step(lambda f) for the first n_sets factors, evaluated in one render_param_sets call per seed
    -> (best candidate, its lambda, its two-seed loss, the largest lambda tried)"""
    lams = [lam * f for f in LAMBDA_FACTORS[:n_sets]]
    cands = np.stack([np.clip(candidate(l), lo, hi) for l in lams])
    ia = render.param_sets(cands, sa).astype(np.float64) - render.target
    ib = render.param_sets(cands, sb).astype(np.float64) - render.target
    losses = (ia * ib).sum((1, 2, 3))
    i = int(np.argmin(losses))
    return cands[i], lams[i], float(losses[i]), max(lams)


STEP_LENGTHS = (1.0, 0.5, 2.0, 0.25)


def cubic_minimiser(a0, f0, g0, a1, f1, g1):
    """the minimiser of the cubic through (a0, f0, slope g0) and (a1, f1, slope g1), g0 < 0 < g1, inside [a0, a1] (Nocedal & Wright 3.59)"""
    d1 = g0 + g1 - 3.0 * (f0 - f1) / (a0 - a1)
    rad = d1 * d1 - g0 * g1
    d2 = np.sqrt(rad) if rad > 0 else 0.0
    a = a1 - (a1 - a0) * (g1 + d2 - d1) / (g1 - g0 + 2.0 * d2)
    t = (a - a0) / (a1 - a0)
    h00, h10, h01, h11 = 2 * t ** 3 - 3 * t ** 2 + 1, t ** 3 - 2 * t ** 2 + t, -2 * t ** 3 + 3 * t ** 2, t ** 3 - t ** 2
    return float(a), float(h00 * f0 + h10 * (a1 - a0) * g0 + h01 * f1 + h11 * (a1 - a0) * g1)


def line_search(render, params, delta, n, sa, sb, lo, hi):
    """n step lengths along delta in one render_param_sets_along call per seed -> (step length, its two-seed loss, "cubic" | "best")"""
    # (no clipping inside the search -- a clipped candidate's derivative would not be the loss's along delta: the lengths shrink instead)
    moving = np.abs(delta) > 0
    room = np.where(delta > 0, hi - params, params - lo)
    scale = min(1.0, float((room[moving] / np.abs(delta[moving])).min()) / max(STEP_LENGTHS[:n])) if moving.any() else 1.0
    alphas = np.sort(np.array(STEP_LENGTHS[:n]) * scale)
    cands = np.stack([params + a * delta for a in alphas])
    dirs = np.stack([delta] * n)
    ia, ta = render.sets_along(cands, dirs, sa)
    ib, tb = render.sets_along(cands, dirs, sb)
    ra, rb = ia.astype(np.float64) - render.target, ib.astype(np.float64) - render.target
    phi = (ra * rb).sum((1, 2, 3))
    slope = (ta.astype(np.float64) * rb + ra * tb.astype(np.float64)).sum((1, 2, 3))
    for i in range(n - 1):
        if slope[i] < 0 < slope[i + 1]:
            a, f = cubic_minimiser(alphas[i], phi[i], slope[i], alphas[i + 1], phi[i + 1], slope[i + 1])
            if f <= min(phi[i], phi[i + 1]):
                return a, f, "cubic"
    i = int(np.argmin(phi))
    return float(alphas[i]), float(phi[i]), "best"


def fit_gauss_newton(render, p_index, start, steps, one_render=False, lam=1e-3, log=None, lambda_sets=0):
    """render as in fit(), plus render.normal_equations(params, seed, residual=None, target=None) -> (A [3,P,P], b [3,P], loss [3], image).
    Levenberg-Marquardt on parameter p_index, per channel.  -> (fitted rgb, history of rgb per step)"""
    params = render.params0.copy()
    params[p_index] = start
    hist = []

    def lm_step(A, b, lam):
        a = A[:, p_index, p_index]
        d = a * (1.0 + lam)
        return np.where(d > 0, -b[:, p_index] / np.where(d > 0, d, 1.0), 0.0)

    for k in range(steps):
        if one_render:
            A, b, loss3, _ = render.normal_equations(params, 1000 + k, target=render.target)
            params[p_index] = np.clip(params[p_index] + lm_step(A, b, lam), 0.0, 1.0)
            loss, verdict = float(loss3.sum()), "one render"
        else:
            img, _ = render(params, 1000 + 2 * k, False, None)
            r = img.astype(np.float64) - render.target
            A, b, _, img_b = render.normal_equations(params, 1001 + 2 * k, residual=r.astype(np.float32))
            loss = float((r * (img_b.astype(np.float64) - render.target)).sum())
            if lambda_sets > 0:
                def candidate(l):
                    c = params.copy()
                    c[p_index] = params[p_index] + lm_step(A, b, l)
                    return c
                hi = np.maximum(1.0, params)
                hi[p_index] = 1.0
                cand, lam_c, loss_c, lam_max = best_of_lambdas(render, params, lam, lambda_sets, 1000 + 2 * k, 1001 + 2 * k, candidate, 0.0, hi)
                if loss_c < loss:
                    params, lam, verdict, loss = cand, max(lam_c / 3.0, 1e-9), "accepted", loss_c      # (logged: the loss the step ends on, as in fit_gauss_newton_along)
                else:
                    lam, verdict = lam_max * 4.0, "rejected"
                hist.append(params[p_index].copy())
                if log:
                    log(f"step {k:3d}  loss {loss:.6f}  lambda {lam:.2e}  {verdict} (best of {lambda_sets})  red = ({params[p_index][0]:.4f}, {params[p_index][1]:.4f}, {params[p_index][2]:.4f})")
                continue
            cand = params.copy()
            cand[p_index] = np.clip(params[p_index] + lm_step(A, b, lam), 0.0, 1.0)
            ca, _ = render(cand, 1000 + 2 * k, False, None)
            ra = ca.astype(np.float64) - render.target          # (a copy: the device renders every forward frame into one pinned buffer)
            cb, _ = render(cand, 1001 + 2 * k, False, None)
            loss_c = float((ra * (cb.astype(np.float64) - render.target)).sum())
            if loss_c < loss:
                params, lam, verdict = cand, max(lam / 3.0, 1e-9), "accepted"
            else:
                lam, verdict = lam * 4.0, "rejected"
        hist.append(params[p_index].copy())
        if log:
            log(f"step {k:3d}  loss {loss:.6f}  lambda {lam:.2e}  {verdict}  red = ({params[p_index][0]:.4f}, {params[p_index][1]:.4f}, {params[p_index][2]:.4f})")
    return params[p_index].copy(), hist


def fit_gauss_newton_cross(render, p_index, start, steps, lam=1e-3, log=None):
    """Levenberg-Marquardt on parameter p_index, per channel, one render_normal_equations_cross call per step (the module's docstring):
    render.normal_equations_cross(params, seed, V) -> (A [3,1,1], b [3,1], loss [3], bias [3,2]).  -> (fitted rgb, history of rgb per step)"""
    params = render.params0.copy()
    params[p_index] = start
    V = np.zeros((1,) + params.shape)
    V[0, p_index] = 1.0                              # (a channel of the radiance depends on the same channel of the albedo alone)
    hist = []
    A, b, loss3, bias = render.normal_equations_cross(params, 1000, V)
    for k in range(steps):
        d = A[:, 0, 0] * (1.0 + lam)
        cand = params.copy()
        cand[p_index] = np.clip(params[p_index] + np.where(d > 0, -b[:, 0] / np.where(d > 0, d, 1.0), 0.0), 0.0, 1.0)
        Ac, bc, lc, biasc = render.normal_equations_cross(cand, 1001 + k, V)
        if float(lc.sum()) < float(loss3.sum()):
            params, A, b, loss3, bias, lam, verdict = cand, Ac, bc, lc, biasc, max(lam / 3.0, 1e-9), "accepted"
        else:
            lam, verdict = lam * 4.0, "rejected"
        hist.append(params[p_index].copy())
        if log:
            log(f"step {k:3d}  loss {float(loss3.sum()):.6f} (noise floor subtracted: {float(bias[:, 1].sum()):.6f})  lambda {lam:.2e}  {verdict}  "
                f"red = ({params[p_index][0]:.4f}, {params[p_index][1]:.4f}, {params[p_index][2]:.4f})")
    return params[p_index].copy(), hist


def fit_gauss_newton_cross_sets(render, p_index, start, steps, n_sets, lam=1e-3, log=None):
    """Levenberg-Marquardt on parameter p_index, per channel, TWO traces per step (the module's docstring): one
    render.normal_equations_cross(params, seed A, V) at the current point, then the candidates of n_sets dampings and the current point
    itself priced on ONE fresh trace, render.param_sets_cross([current, cand_1 ... cand_N], seed B) -> (loss~ [N + 1, 3], bias [N + 1, 3]):
    common paths, each loss unbiased.  The best candidate is accepted iff its loss~ is below the current point's on that same trace.
    -> (fitted rgb, history of rgb per step, per step {"losses": loss~ summed over the channels [N + 1], "best": index, "accepted"})"""
    params = render.params0.copy()
    params[p_index] = start
    V = np.zeros((1,) + params.shape)
    V[0, p_index] = 1.0                              # (a channel of the radiance depends on the same channel of the albedo alone)
    hist, trace = [], []
    for k in range(steps):
        A, b, _, _ = render.normal_equations_cross(params, 1000 + 2 * k, V)
        lams = [lam * f for f in LAMBDA_FACTORS[:n_sets]]
        cands = []
        for l in lams:
            d = A[:, 0, 0] * (1.0 + l)
            c = params.copy()
            c[p_index] = np.clip(params[p_index] + np.where(d > 0, -b[:, 0] / np.where(d > 0, d, 1.0), 0.0), 0.0, 1.0)
            cands.append(c)
        loss3, bias3 = render.param_sets_cross(np.stack([params] + cands), 1001 + 2 * k)
        losses = loss3.sum(1)
        i = 1 + int(np.argmin(losses[1:]))
        accepted = bool(losses[i] < losses[0])
        trace.append({"losses": losses.copy(), "best": i, "accepted": accepted})
        if accepted:
            params, lam, verdict = cands[i - 1], max(lams[i - 1] / 3.0, 1e-9), "accepted"
        else:
            lam, verdict = max(lams) * 4.0, "rejected"
        hist.append(params[p_index].copy())
        if log:
            log(f"step {k:3d}  loss~ {losses[0]:.6f} -> best of {n_sets} {losses[i]:.6f} (noise floors subtracted: {bias3[0].sum():.6f}, {bias3[i].sum():.6f})  "
                f"lambda {lam:.2e}  {verdict}  red = ({params[p_index][0]:.4f}, {params[p_index][1]:.4f}, {params[p_index][2]:.4f})")
    return params[p_index].copy(), hist, trace


def used_params(scene):
    """the parameters some shape's material or emitter refers to (cornell_shapes declares `white` and uses it nowhere: no pixel depends on it)"""
    used = set()
    for _, m, e, _ in scene.shapes:
        if m >= 0:
            used.add(scene.materials[m][1])
        if e >= 0:
            used.add(scene.emitters[e])
    return used


def unit_blocks(n_params, width=8):
    """unit-vector directions (1 on the three channels of one parameter) in blocks of at most `width`: [K, P, 3] each"""
    blocks = []
    for p0 in range(0, n_params, width):
        V = np.zeros((min(width, n_params - p0), n_params, 3))
        for k in range(V.shape[0]):
            V[k, p0 + k, :] = 1.0
        blocks.append(V)
    return blocks


def lm_solve(A, b, lam):
    """per channel (A + lam diag A) x = -b over the rows whose diagonal is positive; the others stay: [K, 3]"""
    K = A.shape[1]
    x = np.zeros((K, 3))
    for ch in range(3):
        d = np.diag(A[ch])
        rows = np.flatnonzero(d > 0)
        if rows.size:
            M = A[ch][np.ix_(rows, rows)] + lam * np.diag(d[rows])
            x[rows, ch] = np.linalg.solve(M, -b[ch][rows])
    return x


def eval_loss(render, params, seeds=(9001, 9002), spp=128):
    """sum over the pixel values of r_A r_B on a fixed pair of sample sets of `spp` samples (not counted as renders of a fit): E = the
    squared error of the true image against the target; the pair's noise falls with 1 / spp"""
    a, _ = render(params, seeds[0], False, None, spp=spp)
    ra = a.astype(np.float64) - render.target
    b, _ = render(params, seeds[1], False, None, spp=spp)
    return float((ra * (b.astype(np.float64) - render.target)).sum())


def fit_gauss_newton_along(render, blocks, start, steps, lam=1e-3, lo=0.0, hi=None, log=None, lambda_sets=0, line_search_n=0):
    """render as in fit(), plus render.normal_equations_along(params, seed, V, residual) -> (A [3,K,K], b [3,K], image).  `blocks`: lists
    of directions [K, P, 3]; per step every block in turn takes a two-seed Levenberg-Marquardt step along its directions (block
    Gauss-Seidel; a lambda per block).  4 renders per block and step.  -> (fitted params, history of the two-seed loss per step)"""
    params = np.array(start, dtype=np.float64)
    hi = np.full(params.shape, 1.0) if hi is None else hi
    lams = [lam] * len(blocks)
    hist = []
    for k in range(steps):
        for bi, V in enumerate(blocks):
            sa, sb = 1000 + 2 * (k * len(blocks) + bi), 1001 + 2 * (k * len(blocks) + bi)
            img, _ = render(params, sa, False, None)
            r = img.astype(np.float64) - render.target
            A, b, img_b = render.normal_equations_along(params, sb, V, r.astype(np.float32))
            loss = float((r * (img_b.astype(np.float64) - render.target)).sum())
            if line_search_n > 0:
                delta = np.einsum("kc,kpc->pc", lm_solve(A, b, lams[bi]), V)
                alpha, loss_c, how = line_search(render, params, delta, line_search_n, sa, sb, lo, hi)
                if loss_c < loss:
                    params, lams[bi], verdict, loss = np.clip(params + alpha * delta, lo, hi), max(lams[bi] / 3.0, 1e-9), "accepted", loss_c
                else:
                    lams[bi], verdict = lams[bi] * 4.0, "rejected"
                if log:
                    log(f"step {k:3d} block {bi}  loss {loss:.6f}  lambda {lams[bi]:.2e}  {verdict} (step length {alpha:.3f}, {how} of {line_search_n})")
                continue
            if lambda_sets > 0:
                cand, lam_c, loss_c, lam_max = best_of_lambdas(render, params, lams[bi], lambda_sets, sa, sb,
                                                               lambda l: params + np.einsum("kc,kpc->pc", lm_solve(A, b, l), V), lo, hi)
                if loss_c < loss:
                    params, lams[bi], verdict, loss = cand, max(lam_c / 3.0, 1e-9), "accepted", loss_c
                else:
                    lams[bi], verdict = lam_max * 4.0, "rejected"
                if log:
                    log(f"step {k:3d} block {bi}  loss {loss:.6f}  lambda {lams[bi]:.2e}  {verdict} (best of {lambda_sets})")
                continue
            x = lm_solve(A, b, lams[bi])
            cand = np.clip(params + np.einsum("kc,kpc->pc", x, V), lo, hi)
            ca, _ = render(cand, sa, False, None)
            ra = ca.astype(np.float64) - render.target
            cb, _ = render(cand, sb, False, None)
            loss_c = float((ra * (cb.astype(np.float64) - render.target)).sum())
            if loss_c < loss:
                params, lams[bi], verdict, loss = cand, max(lams[bi] / 3.0, 1e-9), "accepted", loss_c
            else:
                lams[bi], verdict = lams[bi] * 4.0, "rejected"
            if log:
                log(f"step {k:3d} block {bi}  loss {loss:.6f}  lambda {lams[bi]:.2e}  {verdict}")
        hist.append(loss)
    return params, hist


def fit_adam_all(render, free, start, steps, spp, n_values, lr=0.05, decay=0.97, lo=0.0, hi=None, log=None):
    """Adam on every parameter row listed in `free`, two renders per step as in fit().  -> (fitted params, history of the loss)"""
    params = np.array(start, dtype=np.float64)
    hi = np.full(params.shape, 1.0) if hi is None else hi
    m = np.zeros_like(params); v = np.zeros_like(params)
    b1, b2, eps = 0.8, 0.99, 1e-8
    mask = np.zeros(params.shape[0], bool)
    mask[list(free)] = True
    hist = []
    for k in range(steps):
        img, _ = render(params, 1000 + 2 * k, False, None)
        r = img.astype(np.float64) - render.target
        _, grads = render(params, 1001 + 2 * k, True, (2.0 * r / n_values).astype(np.float32))
        g = np.where(mask[:, None], grads / spp, 0.0)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        params = np.clip(params - lr * decay ** k * (m / (1 - b1 ** (k + 1))) / (np.sqrt(v / (1 - b2 ** (k + 1))) + eps), lo, hi)
        hist.append(float((r ** 2).sum()))
        if log and (k % 4 == 3 or k == steps - 1):
            log(f"adam step {k:3d}  loss {hist[-1]:.6f}")
    return params, hist


MULTI_STEPS = 12      # Adam steps of --multi-start by default


def fit_multi_start(render, free, starts, steps, spp, n_values, lr=0.05, decay=0.97, lo=0.0, hi=None, log=None):
    """fit_adam_all for N chains at once: render.param_sets gives the N images of a step (seed A), render.sets_grad the N gradients (seed
    B, chain k seeded with its own adjoint): two traces per step.  -> (fitted params [N, P, 3], history of the N one-seed losses)"""
    params = np.array(starts, dtype=np.float64)
    hi = np.full(params.shape[1:], 1.0) if hi is None else hi
    m = np.zeros_like(params); v = np.zeros_like(params)
    b1, b2, eps = 0.8, 0.99, 1e-8
    mask = np.zeros(params.shape[1], bool)
    mask[list(free)] = True
    hist = []
    for k in range(steps):
        imgs = render.param_sets(params, 1000 + 2 * k)
        r = imgs.astype(np.float64) - render.target
        grads = render.sets_grad(params, (2.0 * r / n_values).astype(np.float32), 1001 + 2 * k)
        g = np.where(mask[None, :, None], grads / spp, 0.0)
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        params = np.clip(params - lr * decay ** k * (m / (1 - b1 ** (k + 1))) / (np.sqrt(v / (1 - b2 ** (k + 1))) + eps), lo, hi)
        hist.append((r ** 2).sum((1, 2, 3)))
        if log and (k % 4 == 3 or k == steps - 1):
            log(f"multi-start step {k:3d}  losses " + " ".join(f"{x:.6f}" for x in hist[-1]))
    return params, hist


def multi_start(render, n, steps, log=None):
    """n perturbed starts (perturbed_start, seeds 7, 8, ...) as n Adam chains -> dict: the chains' two-seed losses at the start and at the end"""
    P = len(render.params0)
    hi = np.maximum(1.0, render.params0 + 0.5)
    starts = np.stack([perturbed_start(render.params0, seed=7 + i) for i in range(n)])
    calls0 = render.calls
    fitted, hist = fit_multi_start(render, range(P), starts, steps, render.spp, render.target.size, hi=hi, log=log)
    return {"renders": render.calls - calls0, "start_loss": [eval_loss(render, s) for s in starts], "loss": [eval_loss(render, f) for f in fitted],
            "params": fitted, "hist": hist}


def perturbed_start(params0, seed=7, amount=0.2):
    """every value moved by up to `amount`, kept inside (0, 1] for albedos (rows whose true value exceeds 1, the emission, only below by amount)"""
    p = params0 + np.random.RandomState(seed).uniform(-amount, amount, params0.shape)
    return np.clip(p, 0.02, np.maximum(1.0, params0 + amount))


def fit_scene(render, steps, subspace=None, log=None, lambda_sets=0, line_search_n=0):
    """the Levenberg-Marquardt fit of every parameter of render.scene (or of one tint over its albedos) beside Adam with the same number of
    renders, from the same perturbed start -> dict of figures"""
    P = len(render.params0)
    hi = np.maximum(1.0, render.params0 + 0.5)
    if subspace == "tint":
        albedo = [p for p in range(P) if render.params0[p].max() <= 1.0]
        V = np.zeros((3, P, 3))
        for ch in range(3):
            V[ch, albedo, ch] = render.params0[albedo, ch]
        blocks, start, free = [V], render.params0.copy(), albedo
        start[albedo] *= np.array([0.7, 1.25, 0.8])
        start = np.clip(start, 0.0, hi)
    else:
        blocks, start, free = unit_blocks(P), perturbed_start(render.params0), range(P)
    calls0 = render.calls
    fitted, hist = fit_gauss_newton_along(render, blocks, start, steps, hi=hi, log=log, lambda_sets=lambda_sets, line_search_n=line_search_n)
    gn_renders = render.calls - calls0
    calls0 = render.calls
    adam, ahist = fit_adam_all(render, free, start, gn_renders // 2, render.spp, render.target.size, hi=hi, log=log)
    adam_renders = render.calls - calls0
    used = [p for p in free if p in render.used_params()]
    free = used
    return {"start_loss": eval_loss(render, start), "gn_loss": eval_loss(render, fitted), "adam_loss": eval_loss(render, adam),
            "gn_renders": gn_renders, "adam_renders": adam_renders, "gn_steps": steps, "adam_steps": gn_renders // 2,
            "gn_error": float(np.abs(fitted - render.params0)[list(free)].max()), "adam_error": float(np.abs(adam - render.params0)[list(free)].max()),
            "gn_params": fitted, "adam_params": adam, "gn_hist": hist}


class DeviceRender:
    """The device through the C ABI (drt_hip_render, or drt_hip_render_async + drt_hip_wait)."""

    def __init__(self, pkg, size, spp, depth, use_async=False, scene="cornell"):
        self.pkg = pkg
        self.scene = pkg.scene_by_name(scene)
        self.cam = pkg.cornell_camera(size, size)
        self.spp, self.depth, self.use_async = spp, depth, use_async
        self.r = pkg.HipRenderer(0)
        self.r.upload_scene(self.scene)
        self.params0 = np.array(self.scene.params, dtype=np.float64)
        # the loop renders into the same two image buffers (the forward frame's, the gradient frame's), pinned once: the
        # finishing kernel stores a frame straight into its buffer
        self.img = [np.zeros((size, size, 3), dtype=np.float32) for _ in range(2)]
        if not use_async:
            for im in self.img:
                self.r.pin_host(im)
        self.calls = self.traces_of_sets = 0
        self.target, _ = self(self.params0, 1, False, None, spp=256)
        self.target = self.target.astype(np.float64)
        self.calls = 0

    def __call__(self, params, seed, backward, adjoint, spp=None):
        self.r.update_params(params)
        rp = self.pkg.RenderParams(spp=spp or self.spp, min_bounces=self.depth, absorb=1.0, seed=seed)
        self.calls += 1
        if self.use_async:
            img, g, _ = self.r.wait(self.r.render_async(self.cam, rp, backward=backward, adjoint=adjoint), want_stats=False)
        else:
            img, g, _ = self.r.render(self.cam, rp, backward=backward, adjoint=adjoint, img_out=self.img[1 if backward else 0], want_stats=False)
        return img, g

    def normal_equations(self, params, seed, residual=None, target=None):
        self.r.update_params(params)
        rp = self.pkg.RenderParams(spp=self.spp, min_bounces=self.depth, absorb=1.0, seed=seed)
        self.calls += 1
        o = self.r.render_normal_equations(self.cam, rp, target=target, residual=residual)
        return o["A"], o["b"], o["loss"], o["image"]

    def normal_equations_along(self, params, seed, V, residual):
        self.r.update_params(params)
        rp = self.pkg.RenderParams(spp=self.spp, min_bounces=self.depth, absorb=1.0, seed=seed)
        self.calls += 1
        o = self.r.render_normal_equations_along(self.cam, rp, V, residual=residual)
        return o["A"], o["b"], o["image"]

    def normal_equations_cross(self, params, seed, V):
        self.r.update_params(params)
        rp = self.pkg.RenderParams(spp=self.spp, min_bounces=self.depth, absorb=1.0, seed=seed)
        self.calls += 1
        o = self.r.render_normal_equations_cross(self.cam, rp, V, self.target.astype(np.float32))
        return o["A"], o["b"], o["loss"], o["bias"]

    def param_sets(self, sets, seed):
        """the frame under every row of `sets` [N, P, 3] in one trace: [N, H, W, 3]"""
        rp = self.pkg.RenderParams(spp=self.spp, min_bounces=self.depth, absorb=1.0, seed=seed)
        self.calls += 1
        self.traces_of_sets += 1
        return self.r.render_param_sets(self.cam, rp, sets)["images"]

    def param_sets_cross(self, sets, seed):
        """the unbiased loss of every row of `sets` [N, P, 3] against the target, and what was subtracted, in one trace: two of [N, 3]"""
        rp = self.pkg.RenderParams(spp=self.spp, min_bounces=self.depth, absorb=1.0, seed=seed)
        self.calls += 1
        self.traces_of_sets += 1
        o = self.r.render_param_sets_cross(self.cam, rp, sets, self.target.astype(np.float32))
        return o["loss"], o["bias"]

    def sets_along(self, sets, dirs, seed):
        """the frame and its derivative along dirs[k] under every row of `sets` [N, P, 3] in one trace: two of [N, H, W, 3]"""
        rp = self.pkg.RenderParams(spp=self.spp, min_bounces=self.depth, absorb=1.0, seed=seed)
        self.calls += 1
        self.traces_of_sets += 1
        o = self.r.render_param_sets_along(self.cam, rp, sets, dirs)
        return o["images"], o["tangents"]

    def sets_grad(self, sets, adjoints, seed):
        """the summed gradient under every row of `sets` [N, P, 3], row k seeded with adjoints[k], in one trace: [N, P, 3]"""
        rp = self.pkg.RenderParams(spp=self.spp, min_bounces=self.depth, absorb=1.0, seed=seed)
        self.calls += 1
        self.traces_of_sets += 1
        return self.r.render_param_sets_grad(self.cam, rp, sets, adjoints)["grads"]

    def close(self):
        self.r.close()

    def used_params(self):
        return used_params(self.scene)


class OracleRender:
    """TEST INFRASTRUCTURE: the same loop on the CPU restatement."""

    def __init__(self, pkg, oracle, size, spp, depth, scene="cornell"):
        self.pkg, self.oracle = pkg, oracle
        self.calls = self.traces_of_sets = 0
        self.scene = pkg.scene_by_name(scene)
        self.cam = pkg.cornell_camera(size, size)
        self.spp, self.depth = spp, depth
        self.params0 = np.array(self.scene.params, dtype=np.float64)
        self.target, _ = self(self.params0, 1, False, None, spp=256)
        self.calls = 0

    def __call__(self, params, seed, backward, adjoint, spp=None):
        self.calls += 1
        self.scene.params = [tuple(p) for p in params]
        rp = self.pkg.RenderParams(spp=spp or self.spp, min_bounces=self.depth, absorb=1.0, seed=seed)
        o = self.oracle.render(self.scene, self.cam, rp, backward=backward, adjoint=adjoint)
        return o["image"], o["grads"]

    def normal_equations(self, params, seed, residual=None, target=None):
        self.scene.params = [tuple(p) for p in params]
        rp = self.pkg.RenderParams(spp=self.spp, min_bounces=self.depth, absorb=1.0, seed=seed)
        P = len(params)
        J = np.zeros((P,) + self.target.shape)
        img = None
        for p in range(P):
            o = self.oracle.render(self.scene, self.cam, rp, backward=True, grad_image_param=p)
            J[p], img = o["grad_image"], o["image"]
        r = np.asarray(residual, np.float64) if residual is not None else img - np.asarray(target, np.float64)
        return np.einsum("pxyc,qxyc->cpq", J, J), np.einsum("pxyc,xyc->cp", J, r), (r * r).sum((0, 1)), img

    def normal_equations_along(self, params, seed, V, residual):
        """the restatement in place of drt_hip_render_normal_equations_along: T_k = sum_p grad_image(p) v_k[p]"""
        self.calls += 1
        self.scene.params = [tuple(p) for p in params]
        rp = self.pkg.RenderParams(spp=self.spp, min_bounces=self.depth, absorb=1.0, seed=seed)
        T = np.zeros((V.shape[0],) + self.target.shape)
        img = None
        for p in np.flatnonzero(np.abs(V).sum((0, 2)) > 0):
            o = self.oracle.render(self.scene, self.cam, rp, backward=True, grad_image_param=int(p))
            img = o["image"]
            T += np.asarray(o["grad_image"], np.float64)[None] * V[:, p][:, None, None, :]
        r = np.asarray(residual, np.float64)
        return np.einsum("kxyc,lxyc->ckl", T, T), np.einsum("kxyc,xyc->ck", T, r), img

    def param_sets(self, sets, seed):
        """the restatement in place of drt_hip_render_param_sets: a render per set, counted as the one trace it stands for"""
        self.calls += 1
        self.traces_of_sets += 1
        rp = self.pkg.RenderParams(spp=self.spp, min_bounces=self.depth, absorb=1.0, seed=seed)
        out = []
        for p in sets:
            self.scene.params = [tuple(q) for q in p]
            out.append(self.oracle.render(self.scene, self.cam, rp)["image"])
        return np.stack(out)

    def sets_grad(self, sets, adjoints, seed):
        """the restatement in place of drt_hip_render_param_sets_grad: a backward render per set, counted as the one trace it stands for"""
        self.calls += 1
        self.traces_of_sets += 1
        rp = self.pkg.RenderParams(spp=self.spp, min_bounces=self.depth, absorb=1.0, seed=seed)
        out = []
        for p, adj in zip(sets, adjoints):
            self.scene.params = [tuple(q) for q in p]
            out.append(self.oracle.render(self.scene, self.cam, rp, backward=True, adjoint=adj)["grads"])
        return np.stack(out)

    def close(self):
        pass

    def used_params(self):
        return used_params(self.scene)


def arc_cameras(pkg, n, size):
    """n cameras on an arc in front of the box, looking at its middle"""
    cams = []
    for k in range(n):
        t = (k + 0.5) / n - 0.5
        cams.append(pkg.Camera(size, size).look_at((0.5 * np.sin(t), 0.1 * t, 0.15 * (1 - np.cos(t))), (0.0, -0.1, 1.0)))
    return cams


def fit_views(pkg, n_views, size, spp, depth, steps, lr=0.08, decay=0.96, log=None):
    """--views N: fit()'s Adam loop on the red albedo against N target views at once -- per step ONE render_views forward on one seed and ONE
    render_views backward on another, whose summed gradient is the loss's over all views.
    -> (fitted rgb, loss per step, the loss on one fixed seed at 128 spp before and after)"""
    r = pkg.HipRenderer(0)
    scene = pkg.scene_by_name("cornell")
    r.upload_scene(scene)
    cams = arc_cameras(pkg, n_views, size)
    params = np.array(scene.params, dtype=np.float64)
    tracer = dict(min_bounces=depth, absorb=1.0)
    target = r.render_views(cams, pkg.RenderParams(spp=256, seed=1, **tracer))[0].astype(np.float64)
    params[0] = (0.2, 0.2, 0.2)

    def fixed_seed_loss():
        # (the per-step losses are taken on fresh seeds at `spp` and are mostly noise at a few samples: this one compares like with like)
        r.update_params(params)
        imgs = r.render_views(cams, pkg.RenderParams(spp=128, seed=9001, **tracer))[0]
        return float(((imgs.astype(np.float64) - target) ** 2).mean())

    fixed = [fixed_seed_loss()]
    m = np.zeros(3); v = np.zeros(3)
    b1, b2, eps = 0.8, 0.99, 1e-8
    losses = []
    for k in range(steps):
        r.update_params(params)
        imgs = r.render_views(cams, pkg.RenderParams(spp=spp, seed=1000 + 2 * k, **tracer))[0]
        resid = imgs.astype(np.float64) - target
        losses.append(float((resid ** 2).mean()))
        adj = (2.0 * resid / resid.size).astype(np.float32)
        _, gsum, _, _ = r.render_views(cams, pkg.RenderParams(spp=spp, seed=1001 + 2 * k, **tracer), backward=True, adjoints=adj)
        g = gsum[0] / spp
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        params[0] = np.clip(params[0] - lr * decay ** k * (m / (1 - b1 ** (k + 1))) / (np.sqrt(v / (1 - b2 ** (k + 1))) + eps), 0.0, 1.0)
        if log:
            log(f"step {k:3d}  loss {losses[-1]:.6f}  red = ({params[0][0]:.4f}, {params[0][1]:.4f}, {params[0][2]:.4f})")
    fixed.append(fixed_seed_loss())
    r.close()
    return params[0].copy(), losses, fixed


def fit_pixels(pkg, n_views, n_pixels, size, spp, depth, steps, lr=0.08, decay=0.96, log=None, draw_seed=7):
    """--views N --pixels M: fit_views' loop as the stochastic one -- each step draws M (view, pixel) pairs with a seeded generator and makes
    ONE render_pixels forward on one seed and ONE render_pixels backward on another over those pixels alone; the loss of a step is the mean
    squared error over its M entries.
    -> (fitted rgb, loss per step, the loss over ALL views' frames on one fixed seed at 128 spp before and after)"""
    r = pkg.HipRenderer(0)
    scene = pkg.scene_by_name("cornell")
    r.upload_scene(scene)
    cams = arc_cameras(pkg, n_views, size)
    params = np.array(scene.params, dtype=np.float64)
    tracer = dict(min_bounces=depth, absorb=1.0)
    target = r.render_views(cams, pkg.RenderParams(spp=256, seed=1, **tracer))[0].astype(np.float64)
    flat_target = target.reshape(n_views, size * size, 3)
    params[0] = (0.2, 0.2, 0.2)

    def fixed_seed_loss():
        r.update_params(params)
        imgs = r.render_views(cams, pkg.RenderParams(spp=128, seed=9001, **tracer))[0]
        return float(((imgs.astype(np.float64) - target) ** 2).mean())

    fixed = [fixed_seed_loss()]
    rs = np.random.RandomState(draw_seed)
    m = np.zeros(3); v = np.zeros(3)
    b1, b2, eps = 0.8, 0.99, 1e-8
    losses = []
    for k in range(steps):
        r.update_params(params)
        # M (view, pixel) pairs -> the views' lists, one behind the other, and the targets in that order
        view = np.sort(rs.randint(0, n_views, n_pixels))
        pix = rs.randint(0, size * size, n_pixels)
        lists = [pix[view == i] for i in range(n_views)]
        want = flat_target[view, pix]
        rgb = r.render_pixels(cams, lists, pkg.RenderParams(spp=spp, seed=1000 + 2 * k, **tracer))[0]
        resid = rgb.astype(np.float64) - want
        losses.append(float((resid ** 2).mean()))
        adj = (2.0 * resid / resid.size).astype(np.float32)
        _, gsum, _, _ = r.render_pixels(cams, lists, pkg.RenderParams(spp=spp, seed=1001 + 2 * k, **tracer), backward=True, adjoints=adj)
        g = gsum[0] / spp
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        params[0] = np.clip(params[0] - lr * decay ** k * (m / (1 - b1 ** (k + 1))) / (np.sqrt(v / (1 - b2 ** (k + 1))) + eps), 0.0, 1.0)
        if log:
            log(f"step {k:3d}  loss {losses[-1]:.6f}  red = ({params[0][0]:.4f}, {params[0][1]:.4f}, {params[0][2]:.4f})")
    fixed.append(fixed_seed_loss())
    r.close()
    return params[0].copy(), losses, fixed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--steps", type=int, default=None, help="default: 60 (Adam), %d (--gauss-newton)" % GN_STEPS)
    ap.add_argument("--gauss-newton", dest="gauss_newton", action="store_true")
    ap.add_argument("--one-render", dest="one_render", action="store_true")
    ap.add_argument("--cross", action="store_true",
                    help="with --gauss-newton --one-render: b and the loss unbiased from the one render (render_normal_equations_cross)")
    ap.add_argument("--lambda-sets", dest="lambda_sets", type=int, default=0,
                    help="with --gauss-newton: try this many dampings (<= 7) per step in one render_param_sets call per seed")
    ap.add_argument("--line-search", dest="line_search", type=int, default=0,
                    help="with --gauss-newton --scene cornell_shapes: search the step LENGTH over this many candidates (<= 4) in one "
                         "render_param_sets_along call per seed")
    ap.add_argument("--multi-start", dest="multi_start", type=int, default=0,
                    help="with --scene: this many perturbed starts (<= 8) as Adam chains side by side, one render_param_sets and one "
                         "render_param_sets_grad call per step")
    ap.add_argument("--views", type=int, default=0,
                    help="fit the red albedo against this many views (<= 64) on an arc in front of the box: one render_views forward and one "
                         "backward per step; prints the loss per step")
    ap.add_argument("--pixels", type=int, default=0,
                    help="with --views: the stochastic loop -- this many (view, pixel) pairs drawn per step with a seeded generator, one "
                         "render_pixels forward and one backward over them alone")
    ap.add_argument("--async", dest="use_async", action="store_true")
    ap.add_argument("--oracle", action="store_true")
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--scene", default="cornell", help="cornell: the red albedo (the loops above); cornell_shapes: every parameter, with --gauss-newton")
    ap.add_argument("--subspace", choices=("tint",), default=None, help="with --scene cornell_shapes: one tint over the albedos instead of every parameter")
    a = ap.parse_args()
    if a.lambda_sets and (not a.gauss_newton or (a.one_render and not a.cross) or not 1 <= a.lambda_sets <= len(LAMBDA_FACTORS)):
        ap.error("--lambda-sets N (1 ... 7) goes with --gauss-newton (not --one-render, unless with --cross)")
    if a.cross and (not a.gauss_newton or not a.one_render or a.oracle or a.scene != "cornell" or a.spp < 2):
        ap.error("--cross goes with --gauss-newton --one-render on the device, --scene cornell, --spp >= 2")
    if a.line_search and (not a.gauss_newton or a.scene == "cornell" or a.oracle or a.lambda_sets or not 1 <= a.line_search <= len(STEP_LENGTHS)):
        ap.error("--line-search N (1 ... 4) goes with --gauss-newton --scene cornell_shapes on the device (not --oracle, not --lambda-sets)")
    if a.multi_start and (a.gauss_newton or a.use_async or a.lambda_sets or a.line_search or not 1 <= a.multi_start <= 8):
        ap.error("--multi-start N (1 ... 8) is the first-order loop (not --gauss-newton, --async, --lambda-sets, --line-search)")
    if a.views and (a.gauss_newton or a.use_async or a.lambda_sets or a.line_search or a.multi_start or a.oracle or a.scene != "cornell" or
                    not 1 <= a.views <= 64):
        ap.error("--views N (1 ... 64) is the first-order loop on the device, --scene cornell (no other mode)")
    if a.pixels and (not a.views or a.pixels < 1):
        ap.error("--pixels M (>= 1) goes with --views N")
    import __graft_entry__ as e
    pkg = e.load_package()
    if a.views and a.pixels:
        t0 = time.time()
        steps = a.steps or 60
        rgb, losses, fixed = fit_pixels(pkg, a.views, a.pixels, a.size, a.spp, a.depth, steps, log=print)
        print(f"fitted red = ({rgb[0]:.4f}, {rgb[1]:.4f}, {rgb[2]:.4f})  {a.views} views, {a.pixels} pixels a step, {steps} steps, {2 * steps} "
              f"render_pixels calls in {time.time() - t0:.2f} s; loss {losses[0]:.6f} -> {losses[-1]:.6f}; fixed-seed loss {fixed[0]:.6f} -> {fixed[1]:.6f}")
        return 0 if fixed[1] < fixed[0] else 1
    if a.views:
        t0 = time.time()
        steps = a.steps or 60
        rgb, losses, fixed = fit_views(pkg, a.views, a.size, a.spp, a.depth, steps, log=print)
        print(f"fitted red = ({rgb[0]:.4f}, {rgb[1]:.4f}, {rgb[2]:.4f})  {a.views} views, {steps} steps, {2 * steps} render_views calls in "
              f"{time.time() - t0:.2f} s; loss {losses[0]:.6f} -> {losses[-1]:.6f}; fixed-seed loss {fixed[0]:.6f} -> {fixed[1]:.6f}")
        return 0 if fixed[1] < fixed[0] else 1
    if a.oracle:
        render = OracleRender(pkg, e.load_oracle(), a.size, a.spp, a.depth, a.scene)
    else:
        render = DeviceRender(pkg, a.size, a.spp, a.depth, a.use_async, a.scene)
    if a.multi_start:
        t0 = time.time()
        f = multi_start(render, a.multi_start, a.steps or MULTI_STEPS, log=None if a.quiet else print)
        for i, (l0, l1) in enumerate(zip(f["start_loss"], f["loss"])):
            print(f"chain {i}: two-seed loss {l0:.5f} at its start, {l1:.5f} after {a.steps or MULTI_STEPS} steps")
        best = int(np.argmin(f["loss"]))
        print(f"{a.scene}: {a.multi_start} Adam chains, {f['renders']} renders ({render.traces_of_sets} of them traces of {a.multi_start} sets: two per "
              f"step where separate runs take {2 * a.multi_start}); best chain {best}: loss {f['loss'][best]:.5f}  ({time.time() - t0:.2f} s)")
        return 0 if all(l1 < l0 for l0, l1 in zip(f["start_loss"], f["loss"])) else 1
    if a.scene != "cornell":
        if not a.gauss_newton:
            ap.error("--scene other than cornell goes with --gauss-newton")
        t0 = time.time()
        f = fit_scene(render, a.steps or ALONG_STEPS, a.subspace, log=None if a.quiet else print, lambda_sets=a.lambda_sets, line_search_n=a.line_search)
        if a.line_search:
            print(f"--line-search {a.line_search}: {render.traces_of_sets} of the renders were traces of {a.line_search} step lengths")
        if a.lambda_sets:
            print(f"--lambda-sets {a.lambda_sets}: {render.traces_of_sets} of the renders were traces of {a.lambda_sets} candidates")
        print(f"{a.scene}{' (tint)' if a.subspace else ''}: two-seed loss at the start {f['start_loss']:.5f}; Levenberg-Marquardt {f['gn_steps']} steps, "
              f"{f['gn_renders']} renders: loss {f['gn_loss']:.5f}, max parameter error {f['gn_error']:.4f}; Adam {f['adam_steps']} steps, "
              f"{f['adam_renders']} renders: loss {f['adam_loss']:.5f}, max parameter error {f['adam_error']:.4f}  ({time.time() - t0:.2f} s)")
        return 0 if f["gn_loss"] < f["adam_loss"] else 1
    if a.steps is None:
        a.steps = GN_STEPS if a.gauss_newton else 60
    if a.gauss_newton:
        t0 = time.time()
        if a.cross and a.lambda_sets:
            rgb, hist, _ = fit_gauss_newton_cross_sets(render, 0, np.array([0.2, 0.2, 0.2]), a.steps, a.lambda_sets, log=None if a.quiet else print)
        elif a.cross:
            rgb, hist = fit_gauss_newton_cross(render, 0, np.array([0.2, 0.2, 0.2]), a.steps, log=None if a.quiet else print)
        else:
            rgb, hist = fit_gauss_newton(render, 0, np.array([0.2, 0.2, 0.2]), a.steps, a.one_render, log=None if a.quiet else print,
                                         lambda_sets=a.lambda_sets)
        dt = time.time() - t0
        if a.lambda_sets:
            print(f"--lambda-sets {a.lambda_sets}: {render.traces_of_sets} of the renders below were traces of {a.lambda_sets} candidates each")
        err = np.abs(rgb - np.array([0.5, 0.0, 0.0])).max()
        n = (2 * a.steps if a.lambda_sets else (a.steps + 1 if a.cross else a.steps)) if a.one_render else 4 * a.steps
        print(f"fitted red = ({rgb[0]:.4f}, {rgb[1]:.4f}, {rgb[2]:.4f})  max error {err:.4f}  "
              f"{a.steps} Gauss-Newton steps, {n} renders in {dt:.2f} s")
        return 0 if err <= 1e-2 else 1
    t0 = time.time()
    rgb, hist = fit(render, len(render.params0), 0, np.array([0.2, 0.2, 0.2]), a.steps, a.spp, a.size * a.size * 3,
                    log=None if a.quiet else print)
    dt = time.time() - t0
    err = np.abs(rgb - np.array([0.5, 0.0, 0.0])).max()
    print(f"fitted red = ({rgb[0]:.4f}, {rgb[1]:.4f}, {rgb[2]:.4f})  max error {err:.4f}  "
          f"{a.steps} steps, {2 * a.steps} renders in {dt:.2f} s ({1e3 * dt / (2 * a.steps):.2f} ms per render"
          f"{', drt_hip_render_async + drt_hip_wait' if a.use_async else ''})")
    return 0 if err <= 1e-2 else 1


if __name__ == "__main__":
    sys.exit(main())
