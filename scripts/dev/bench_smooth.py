#!/usr/bin/env python
"""
Times the two pose filters of csrc/smooth.hip (`empose_smooth_window`, `empose_smooth_one_euro`) against their restatement
in float64 torch on the same GPU, at rows of 22 joints and 10 channels:

  shapes      36 recordings x 1501 frames (offline evaluation) and 1024 windows x 32 frames (a training-size batch)
  window      Gaussian taps at R = 8 and R = 32
  one-euro    the whole sequences in one call, and one frame per call with the state carried (F = 1: streaming)

  kernel      `em_pose_amd.eval.smoothing.smooth_window` / `OneEuroFilter`
  torch       the same definitions from slices in float64: the window as a loop over k on whole tensors, the One-Euro
              filter as a loop over the frames (it is a recurrence)

Every frame counts (the restatements have no validity handling).  Per row: 10 warm-up calls, then 40 timed calls, each
measured with device events and with the host clock around the call plus a final synchronisation; the medians are printed.
The torch One-Euro loop over 1501 frames takes most of a second per call and is timed over 3 calls after 1.  The table is
measured three times in turn (rounds).  The peak allocated bytes of a call above its inputs are measured on one further
call per row.  Before anything is timed the two routes are compared (rotations by geodesic angle).

    python scripts/dev/bench_smooth.py [--out profiles/smooth_mi355x.txt]
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from em_pose_amd.eval.smoothing import OneEuroFilter, gaussian_taps, smooth_window  # noqa: E402

ROUNDS = 3
FPS, J, C = 60.0, 22, 10
SHAPES = ((36, 1501), (1024, 32))
EURO = dict(min_cutoff=1.0, beta=0.5, d_cutoff=1.0)


def timed(fn, calls=40, warmup=10):
    ev, wall = [], []
    for it in range(warmup + calls):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it >= warmup:
            ev.append(a.elapsed_time(b))
            wall.append((t1 - t0) * 1e3)
    return float(np.median(ev)), float(np.median(wall))


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


# ---- float64 torch restatements (every frame counts) -----------------------------------------------------------------------
def quat(r):
    t = torch.linalg.norm(r, dim=-1, keepdim=True)
    k = torch.where(t < 1e-8, torch.full_like(t, 0.5), torch.sin(0.5 * t) / t.clamp_min(1e-300))
    return torch.cat([torch.cos(0.5 * t), k * r], dim=-1)


def rotvec(q):
    q = torch.where(q[..., :1] < 0, -q, q)
    s = torch.linalg.norm(q[..., 1:], dim=-1, keepdim=True)
    k = torch.where(s < 1e-8, torch.full_like(s, 2.0), 2.0 * torch.atan2(s, q[..., :1]) / s.clamp_min(1e-300))
    return k * q[..., 1:]


def qmul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], dim=-1)


def torch_window(rows, taps):
    n, f = rows.shape[:2]
    x = rows.double()
    q, lin = quat(x[..., :3 * J].reshape(n, f, J, 3)), x[..., 3 * J:]
    acc_q, acc_l = taps[0] * q, taps[0] * lin
    wsum = torch.full((1, f, 1), float(taps[0]), dtype=torch.float64, device=rows.device)
    for k in range(1, min(len(taps) - 1, (f - 1) // 2) + 1):
        c, p, s = q[:, k:f - k], q[:, :f - 2 * k], q[:, 2 * k:]
        sp = torch.where((c * p).sum(-1, keepdim=True) < 0, -1.0, 1.0)
        ss = torch.where((c * s).sum(-1, keepdim=True) < 0, -1.0, 1.0)
        acc_q[:, k:f - k] += taps[k] * (sp * p + ss * s)
        acc_l[:, k:f - k] += taps[k] * (lin[:, :f - 2 * k] + lin[:, 2 * k:])
        wsum[:, k:f - k] += 2.0 * taps[k]
    rot = rotvec(acc_q / torch.linalg.norm(acc_q, dim=-1, keepdim=True)).reshape(n, f, 3 * J)
    return torch.cat([rot, acc_l / wsum], dim=-1)


def alpha(fc):
    return 1.0 / (1.0 + FPS / (2.0 * math.pi * fc))


def torch_one_euro(rows, state=None):
    """-> (out, state); state = (x^ quaternions, x^ channels, s^ rotations, s^ channels) or None (fresh)."""
    n, f = rows.shape[:2]
    x = rows.double()
    out = torch.empty_like(x)
    a_d = alpha(EURO['d_cutoff'])
    for t in range(f):
        q, lin = quat(x[:, t, :3 * J].reshape(n, J, 3)), x[:, t, 3 * J:]
        if state is None:
            xq, xl = q, lin
            sq, sl = torch.zeros_like(q[..., 0]), torch.zeros_like(lin)
        else:
            xq, xl, sq, sl = state
            q = torch.where((xq * q).sum(-1, keepdim=True) < 0, -q, q)
            rel = qmul(xq * xq.new_tensor([1.0, -1.0, -1.0, -1.0]), q)
            s = torch.linalg.norm(rel[..., 1:], dim=-1, keepdim=True)
            delta = torch.atan2(s, rel[..., :1]) / s.clamp_min(1e-300) * rel[..., 1:]
            half = torch.linalg.norm(delta, dim=-1)
            sq = sq + a_d * (2.0 * half * FPS - sq)
            step = alpha(EURO['min_cutoff'] + EURO['beta'] * sq.abs())[..., None] * delta
            a = torch.linalg.norm(step, dim=-1, keepdim=True)
            e = torch.cat([torch.cos(a), torch.where(a < 1e-8, torch.ones_like(a), torch.sin(a) / a.clamp_min(1e-300)) * step],
                          dim=-1)
            y = qmul(xq, e)
            xq = y / torch.linalg.norm(y, dim=-1, keepdim=True)
            sl = sl + a_d * ((lin - xl) * FPS - sl)
            xl = xl + alpha(EURO['min_cutoff'] + EURO['beta'] * sl.abs()) * (lin - xl)
        state = (xq, xl, sq, sl)
        out[:, t, :3 * J] = rotvec(xq).reshape(n, 3 * J)
        out[:, t, 3 * J:] = xl
    return out, state


def inputs(n, f, dev):
    """Smooth rotation walks (0.04 rad per frame about a fixed axis per joint) plus 0.02 rad of noise; channels below 2."""
    gen = torch.Generator().manual_seed(n * 10000 + f)
    axis = torch.nn.functional.normalize(torch.randn(n, 1, J, 3, generator=gen, dtype=torch.float64), dim=-1)
    t = torch.arange(f, dtype=torch.float64)[None, :, None, None]
    base = quat(torch.randn(n, 1, J, 3, generator=gen, dtype=torch.float64)).expand(n, f, J, 4)
    q = qmul(qmul(base, quat(0.04 * t * axis)), quat(0.02 * torch.nn.functional.normalize(
        torch.randn(n, f, J, 3, generator=gen, dtype=torch.float64), dim=-1)))
    lin = 1.7 * torch.sin(2 * math.pi * torch.rand(n, 1, C, generator=gen, dtype=torch.float64) * 2.0 * t[..., 0] / FPS) + \
        0.05 * torch.randn(n, f, C, generator=gen, dtype=torch.float64)
    return torch.cat([rotvec(q).reshape(n, f, 3 * J), lin], dim=-1).float().contiguous().to(dev)


def difference(got, want):
    """(largest geodesic angle between the rotations, rad; largest difference of the channels)."""
    n, f = got.shape[:2]
    a, b = quat(got[..., :3 * J].double().reshape(n, f, J, 3)), quat(want[..., :3 * J].reshape(n, f, J, 3))
    rel = qmul(a * a.new_tensor([1.0, -1.0, -1.0, -1.0]), b)
    ang = 2.0 * torch.atan2(torch.linalg.norm(rel[..., 1:], dim=-1), rel[..., 0].abs())
    return float(ang.max()), float((got[..., 3 * J:].double() - want[..., 3 * J:]).abs().max())


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X: a timing without the GPU says nothing')
    dev = torch.device('cuda:0')
    lines = ['pose smoothing (empose_smooth_window, empose_smooth_one_euro) on {} ({}), rows of {} joints + {} channels:'.format(
                 torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName, J, C),
             'median of 40 calls after 10 warm-up calls (torch one-euro over whole sequences: 3 after 1), milliseconds; median '
             'over {} rounds [lowest .. highest round]; peak: bytes allocated by one call above its inputs'.format(ROUNDS)]
    fmt = lambda x: '{:.4f} [{:.4f} .. {:.4f}]'.format(float(np.median(x)), min(x), max(x))
    for n, f in SHAPES:
        rows = inputs(n, f, dev)
        cases = []
        for R in (8, 32):
            taps = [float(w) for w in gaussian_taps(R / 2.0, radius=R)]
            cases.append(('window R = {}'.format(R), lambda taps=taps: smooth_window(rows, None, taps, J, C),
                          lambda taps=taps: torch_window(rows, taps), {}))
        filt = OneEuroFilter(J, C, fps=FPS, **EURO)
        cases.append(('one-euro, whole', lambda: filt(rows), lambda: torch_one_euro(rows)[0], dict(calls=3, warmup=1)))
        # one frame per call with the state carried: the state after the first frame, then the second frame again and again
        filt1 = OneEuroFilter(J, C, fps=FPS, **EURO)
        filt1(rows[:, :1])
        state1 = filt1._state.clone()
        _, tstate = torch_one_euro(rows[:, :1])

        def kernel_step():
            filt1._state = state1
            return filt1(rows[:, 1:2], is_new_sequence=False)
        cases.append(('one-euro, F = 1', kernel_step, lambda: torch_one_euro(rows[:, 1:2], tstate)[0], {}))
        lines.append('{} x {} frames, input {:.2f} MB'.format(n, f, rows.numel() * 4 / 1e6))
        lines.append('{:<18} {:<8} {:>32} {:>32} {:>14}   {}'.format('', '', 'events', 'wall', 'peak bytes',
                                                                     'kernel against torch: rotations rad, channels'))
        for name, kernel, restated, how in cases:
            ang, lin = difference(kernel(), restated())
            assert ang <= 1e-6 and lin <= 1e-6, (name, ang, lin)
            res = {'kernel': [], 'torch': []}
            for _ in range(ROUNDS):
                res['kernel'].append(timed(kernel))
                res['torch'].append(timed(restated, **how))
            for k, fn in (('kernel', kernel), ('torch', restated)):
                lines.append('{:<18} {:<8} {:>32} {:>32} {:>14d}   {}'.format(
                    name, k, fmt([r[0] for r in res[k]]), fmt([r[1] for r in res[k]]), peak_bytes(fn),
                    '{:.2e}, {:.2e}'.format(ang, lin) if k == 'kernel' else ''))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
