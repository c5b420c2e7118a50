#!/usr/bin/env python
"""
Times the two modes of `empose_temporal_rows` (csrc/temporal.hip) against their restatement in torch on the same GPU:

  per-point   54 030 frames (the frame count of the EM-POSE test set) x 22 joints, one row:  rows (frames, 66) float64
  reduced     1027 frames x 6890 vertices (one mesh slab of the engine plus its lead-in):     rows (frames, 6) float64

  kernel      `em_pose_amd.eval.temporal_metrics.temporal_rows`: one launch, each value loaded once
  torch       the same figures from slices in float64 (`x[:, 3:] - 3 x[:, 2:-1] + ...`, `norm`, `sum`)

Every frame counts (the torch restatement has no validity handling).  Per row: 10 warm-up calls, then 40 timed calls, each
measured with device events and with the host clock around the call plus a final synchronisation; the medians are printed.
The table is measured three times in turn (rounds).  The peak allocated bytes of a call above its inputs are measured on
one further call per row.  Before anything is timed the two routes are compared.

    python scripts/dev/bench_temporal_metrics.py [--out profiles/temporal_metrics_mi355x.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from em_pose_amd import synthetic  # noqa: E402
from em_pose_amd.eval.temporal_metrics import temporal_rows  # noqa: E402

ROUNDS = 3
FPS = 60.0
CASES = (('per-point', int(sum(synthetic.README_SEQUENCE_LENGTHS)), 22, False), ('reduced', 1027, 6890, True))


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


def torch_rows(g, h, reduce):
    """(1, f, P, 3) float32 -> (f, 3 P) float64, or (f, 6) with `reduce`; the first frames, where nothing is defined, are 0."""
    g, h = g.double(), h.double()
    acc = lambda x: (x[:, 2:] - 2.0 * x[:, 1:-1] + x[:, :-2]) * FPS ** 2
    jerk = lambda x: (x[:, 3:] - 3.0 * x[:, 2:-1] + 3.0 * x[:, 1:-2] - x[:, :-3]) * FPS ** 3
    pad = lambda t, k: torch.cat([torch.zeros(k, t.shape[1], dtype=t.dtype, device=t.device), t])
    parts = [pad(torch.linalg.norm(acc(g) - acc(h), dim=-1)[0], 2), pad(torch.linalg.norm(jerk(h), dim=-1)[0], 3),
             pad(torch.linalg.norm(jerk(g), dim=-1)[0], 3)]
    if not reduce:
        return torch.cat(parts, dim=1)
    return torch.stack([s for p_ in parts for s in (p_.sum(dim=1), (p_ * p_).sum(dim=1))], dim=1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X: a timing without the GPU says nothing')
    dev = torch.device('cuda:0')
    lines = ['temporal metrics rows (empose_temporal_rows) on {} ({}):'.format(
                 torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName),
             'median of 40 calls after 10 warm-up calls, milliseconds; median over {} rounds [lowest .. highest round]; '
             'peak: bytes allocated by one call above its inputs'.format(ROUNDS)]
    fmt = lambda x: '{:.4f} [{:.4f} .. {:.4f}]'.format(float(np.median(x)), min(x), max(x))
    for name, f, P, reduce in CASES:
        gen = torch.Generator().manual_seed(f)
        t = torch.arange(f, dtype=torch.float64)[:, None, None] / FPS
        hz, ph = torch.rand(1, P, 3, generator=gen, dtype=torch.float64) * 2.5 + 0.5, torch.rand(1, P, 3, generator=gen,
                                                                                                 dtype=torch.float64) * 6.28
        g = (0.5 * torch.sin(6.283185307179586 * hz * t + ph)).float()[None].contiguous()
        h = g + torch.randn(g.shape, generator=gen) * 1e-3
        g, h = g.to(dev), h.to(dev)
        valid = torch.ones(1, f, dtype=torch.uint8, device=dev)
        kernel = lambda: temporal_rows(g, h, valid, FPS, reduce=reduce)[0]
        restated = lambda: torch_rows(g, h, reduce)
        a, b = kernel()[0], restated()
        diff = float(((a - b).abs() / b.abs().clamp_min(1.0)).max())
        assert diff <= 1e-9, diff
        rows = (('kernel', kernel), ('torch', restated))
        res = {k: [] for k, _ in rows}
        for _ in range(ROUNDS):
            for k, fn in rows:
                res[k].append(timed(fn))
        lines.append('{}: {} frames x {} points, inputs {:.1f} MB, rows {:.1f} MB; kernel against torch, largest relative '
                     'difference {:.3e}'.format(name, f, P, 2 * g.numel() * 4 / 1e6, a.numel() * 8 / 1e6, diff))
        lines.append('{:<10} {:>32} {:>32} {:>16}'.format('', 'events', 'wall', 'peak bytes'))
        for k, fn in rows:
            lines.append('{:<10} {:>32} {:>32} {:>16d}'.format(k, fmt([r[0] for r in res[k]]), fmt([r[1] for r in res[k]]),
                                                              peak_bytes(fn)))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
