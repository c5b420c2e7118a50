#!/usr/bin/env python
"""
Times ground-truth preprocessing after root normalisation -- `fn(batch, mode='after_normalize')` of
`get_end_to_end_preprocess_fn`: SMPLFK -> SampleMarkersWithOffsets -- on the V = 6890 synthetic body model at 12 x 32 and
256 x 32 windows, offset noise levels -1 and 1, in four configurations: the switches-off path (full mesh, torch
offsets), `device_offsets` (one launch of empose_sample_sensors_fwd), `sensors_only` (the sensor sub-mesh instead of
the full mesh) and both.  Per configuration: 10 warm-up calls, then 40 timed calls, each measured with device events and
with the host clock around the call plus a final synchronisation; the medians are printed, with the peak of the bytes
allocated during a call.  The whole table is measured three times in turn (rounds); the spread of a median over the
rounds is the run-to-run spread a difference has to exceed.

    python scripts/dev/bench_sample_sensors.py [--out profiles/sample_sensors_mi355x.txt]
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
from em_pose_amd.bodymodels.smpl import SMPLLayer  # noqa: E402
from em_pose_amd.data.data import AMASSBatch, AMASSSample  # noqa: E402
from em_pose_amd.data.transforms import ToTensor, get_end_to_end_preprocess_fn  # noqa: E402
from em_pose_amd.helpers.configuration import CONSTANTS as C, lgd_config  # noqa: E402

CONFIGS = (('parent path', False, False), ('device_offsets', True, False), ('sensors_only', False, True),
           ('both', True, True))
ROUNDS = 3


def make_batch(n, f, dev):
    rng = np.random.default_rng(n)
    samples = [ToTensor()(AMASSSample('s%d' % i, rng.normal(0, 0.2, size=(f, 66)).astype(np.float32),
                                      rng.normal(0, 1, size=10).astype(np.float32),
                                      np.zeros((f, 3), np.float32), 60.0)) for i in range(n)]
    return AMASSBatch.from_sample_list(samples).to_gpu(dev)


def timed(fn, batch, calls=40, warmup=10):
    ev, wall, peak = [], [], 0
    for it in range(warmup + calls):
        torch.cuda.synchronize()
        if it == warmup:
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn(batch, mode='after_normalize')
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it >= warmup:
            ev.append(a.elapsed_time(b))
            wall.append((t1 - t0) * 1e3)
            peak = max(peak, torch.cuda.max_memory_allocated() - base)
    return float(np.median(ev)), float(np.median(wall)), peak


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X: a timing without the GPU says nothing')
    dev = torch.device('cuda:0')
    smpl = SMPLLayer(synthetic.make_model()).to(dev)
    rng = np.random.default_rng(0)
    offsets = [{'means': rng.normal(0, 0.02, size=(12, 3)).astype(np.float32),
                'covs': np.tile(np.eye(3, dtype=np.float32) * 1e-4, (12, 1, 1)),
                'r': np.linalg.qr(rng.normal(size=(12, 3, 3)))[0].astype(np.float32),
                'vertex_ids': np.asarray(C.VERTEX_IDS)} for _ in range(3)]
    lines = ['ground-truth preprocessing after normalisation (SMPLFK -> SampleMarkersWithOffsets), V = 6890, on {}:'.format(
        torch.cuda.get_device_name(0)),
        'median of 40 calls after 10 warm-up calls, milliseconds; median over {} rounds [lowest .. highest round]; peak bytes '
        'allocated during a call'.format(ROUNDS),
        '{:<10} {:>5} {:<15} {:>30} {:>30} {:>14}'.format('windows', 'level', 'configuration', 'events', 'wall', 'peak bytes')]
    for n, f in ((12, 32), (256, 32)):
        batch = make_batch(n, f, dev)
        for level in (-1, 1):
            cfg = lgd_config(12, True, 2, offset_noise_level=level)
            fns = {name: get_end_to_end_preprocess_fn(cfg, smpl, offsets, randomize_if_configured=level >= 0,
                                                      device_offsets=d, sensors_only=s) for name, d, s in CONFIGS}
            # the same seeds: the same draws; the outputs agree before anything is timed
            outs = {}
            for name, fn in fns.items():
                torch.manual_seed(0)
                fn.sample_markers.offset_rng = np.random.RandomState(6273)
                o = fn(batch, mode='after_normalize')
                outs[name] = (o.marker_pos_synth.clone(), o.marker_ori_synth.clone())
            for name in fns:
                for a, b in zip(outs[name], outs['parent path']):
                    assert float((a - b).abs().max()) <= 2e-5, name
            res = {name: [] for name in fns}
            for _ in range(ROUNDS):
                for name, fn in fns.items():
                    res[name].append(timed(fn, batch))
            for name in fns:
                ev, wall = [r[0] for r in res[name]], [r[1] for r in res[name]]
                fmt = lambda x: '{:.4f} [{:.4f} .. {:.4f}]'.format(float(np.median(x)), min(x), max(x))
                lines.append('{:<10} {:>5} {:<15} {:>30} {:>30} {:>14}'.format(
                    '{} x {}'.format(n, f), level, name, fmt(ev), fmt(wall), max(r[2] for r in res[name])))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
