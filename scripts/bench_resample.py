#!/usr/bin/env python
"""
Times the resampling entry points (csrc/resample.hip) on the GPU with device events, median of `--calls` calls after a
warm-up, tables uploaded and buffers allocated beforehand:

  * one 120 Hz sequence of 36 000 frames (5 minutes) to 60 Hz, 22 joints / 3 translation channels;
  * a ragged batch of 256 sequences of 1 000 - 10 000 frames (seeded lengths, rates drawn from 100 / 120 / 250 Hz).

Beside them the float64 NumPy restatement of the rotation side (tests/resample_ref.py) and scipy's CubicSpline on the host
for the single sequence, once each.  Prints one line per number.

    python scripts/bench_resample.py [--calls 40] [--no_host]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from em_pose_amd import _lib  # noqa: E402
from em_pose_amd.data import resample as RS  # noqa: E402


def timed(fn, calls, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def case(name, lengths, rates, calls, dev, rng):
    lib = _lib.lib()
    table = RS.sequence_table(lengths, rates, 60.0)
    rows_in, rows_out = int(sum(lengths)), int(table['f_out'].sum())
    dev_table = torch.from_numpy(table.view(np.uint8)).to(dev)
    host = table.ctypes.data_as(_lib.C.c_void_p)
    rot = torch.from_numpy(np.cumsum(rng.normal(0, 0.05, (rows_in, 66)), axis=0).astype(np.float32)).to(dev)
    pos = torch.from_numpy((2.0 + np.cumsum(rng.normal(0, 0.02, (rows_in, 3)), axis=0)).astype(np.float32)).to(dev)
    rot_out = torch.empty(rows_out, 66, device=dev)
    pos_out = torch.empty(rows_out, 3, device=dev)
    ws_bytes = lib.empose_resample_positions_workspace_bytes(rows_in, 3)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    stream = _lib.current_stream()
    f_rot = lambda: _lib.check(lib.empose_resample_rotations(len(table), host, _lib.dptr(dev_table), 22, _lib.dptr(rot), 66,
                                                             rows_in, _lib.dptr(rot_out), 66, rows_out, stream))
    f_pos = lambda: _lib.check(lib.empose_resample_positions(len(table), host, _lib.dptr(dev_table), 3, _lib.dptr(pos), 3,
                                                             rows_in, _lib.dptr(pos_out), 3, rows_out, _lib.dptr(ws),
                                                             ws_bytes, stream))
    for what, fn in (('rotations (22 joints)', f_rot), ('positions (3 channels)', f_pos)):
        med, lo, hi = timed(fn, calls)
        print('{}: {} sequences, {} -> {} frames, {}: median {:.4f} ms (min {:.4f}, max {:.4f}) over {} calls'
              .format(name, len(lengths), rows_in, rows_out, what, med, lo, hi, calls), flush=True)
    return rot, pos


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--calls', type=int, default=40)
    p.add_argument('--no_host', action='store_true')
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_resample.py measures on the GPU; there is nothing to measure without one.')
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(60)
    print('device:', torch.cuda.get_device_name(dev), flush=True)
    rot, pos = case('single', [36000], 120.0, args.calls, dev, rng)
    lengths = rng.integers(1000, 10001, 256).tolist()
    case('ragged', lengths, rng.choice([100.0, 120.0, 250.0], 256), args.calls, dev, rng)
    if not args.no_host:
        from scipy.interpolate import CubicSpline
        from tests import resample_ref as RR
        r, x = rot.cpu().numpy().reshape(36000, 22, 3), pos.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        RR.resample_rotations(r, 120.0, 60.0)
        print('single: host float64 NumPy restatement, rotations: {:.1f} ms'.format((time.perf_counter() - t0) * 1e3))
        t0 = time.perf_counter()
        CubicSpline(np.arange(0, 300.0, 1 / 120.0)[:36000], x, axis=0)(np.arange(0, 300.0, 1 / 60.0))
        print('single: host scipy CubicSpline, positions: {:.1f} ms'.format((time.perf_counter() - t0) * 1e3))


if __name__ == '__main__':
    main()
