"""
Generates tests/golden/sensor_noise.npz by running the UNMODIFIED reference classes
(`empose.data.noise_functions.SphericalMarkerNoise`, `MarkerSuppressionNoise`) on the CPU.  Run from the repository root:

    python tests/golden/make_golden_sensor_noise.py <path of a checkout of the reference>

Nothing from the reference is copied: the script imports it, feeds it seeded inputs and stores, per case, the draws its
generators gave (recorded at torch.randperm / torch.randint / torch.rand while the reference runs) and the three
outputs.  The inputs are shared by all cases: N = 5 windows, F = 16 frames, M = 12 sensors.  Every case is two
consecutive calls of ONE object, so the second call's draws record what the generators carry over.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, 'tests', 'golden', 'sensor_noise.npz')
N, F, M = 5, 16, 12

# name: (kind, constructor arguments of the reference class)
CASES = {
    'spherical_a': ('spherical', dict(sphere_size=0.5, window_size=0.25, num_markers=1)),
    'spherical_b': ('spherical', dict(sphere_size=1.0, window_size=1.0, num_markers=12)),
    'suppress_a': ('suppress', dict(window_size=0.3, num_markers=1, mask_value=0.0, n_markers_in=12)),
    'suppress_b': ('suppress', dict(window_size=1.0, num_markers=3, mask_value=-2.5, n_markers_in=6)),
}


def inputs():
    """Sensor readings of the size of a body: sites within a metre of the origin that move a few centimetres, the right
    upper and lower leg sensors 0.42 m apart (the thigh the spherical noise measures), rotations for the orientations."""
    rng = np.random.default_rng(20240607)
    base = rng.uniform(-0.8, 0.8, size=(M, 3))
    base[5], base[6] = (-0.10, -0.30, 0.05), (-0.12, -0.72, 0.0)
    pos = base[None, None] + rng.normal(0, 0.03, size=(N, F, M, 3))
    q = rng.normal(size=(N, F, M, 4))
    q /= np.linalg.norm(q, axis=-1, keepdims=True)
    w, x, y, z = np.moveaxis(q, -1, 0)
    ori = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                    2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                    2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1).reshape(N, F, M, 3, 3)
    f32 = lambda a, c: np.ascontiguousarray(a.reshape(N, F, M * c), dtype=np.float32)
    return f32(pos, 3), f32(ori, 9), f32(ori[..., 2], 3)


class Recorder(object):
    """Records what torch.randperm / randint / rand return while it is active; the functions themselves are torch's."""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        self.saved = {k: getattr(torch, k) for k in ('randperm', 'randint', 'rand')}
        for k, fn in self.saved.items():
            setattr(torch, k, self._wrap(k, fn))
        return self

    def _wrap(self, name, fn):
        def wrapped(*a, **kw):
            out = fn(*a, **kw)
            self.calls.append((name, out.clone()))
            return out
        return wrapped

    def __exit__(self, *exc):
        for k, fn in self.saved.items():
            setattr(torch, k, fn)
        return False


def main(ref):
    tmp = tempfile.mkdtemp()
    for k in ('EM_DATA_SYNTH', 'EM_EXPERIMENTS', 'SMPL_MODELS', 'EM_DATA_REAL'):   # read when the reference is imported
        os.environ.setdefault(k, tmp)
    sys.path.insert(0, ref)
    from empose.data import noise_functions as NF
    from empose.helpers.configuration import CONSTANTS as RC

    pos, ori, normal = inputs()
    data = {'pos': pos, 'ori': ori, 'normal': normal,
            'thigh_idx': np.asarray([RC.T_TO_IDX_WO_ROOT[RC.T_RUL], RC.T_TO_IDX_WO_ROOT[RC.T_RLL]], np.int32)}
    for name, (kind, kw) in CASES.items():
        fn = NF.SphericalMarkerNoise(**kw) if kind == 'spherical' else NF.MarkerSuppressionNoise(**kw)
        torch.manual_seed(4711)   # the radii of the spherical noise come from the global generator
        for call in (0, 1):
            batch = types.SimpleNamespace(marker_pos_synth=torch.from_numpy(pos.copy()),
                                          marker_ori_synth=torch.from_numpy(ori.copy()),
                                          marker_normal_synth=torch.from_numpy(normal.copy()),
                                          marker_pos_noisy=None, marker_ori_noisy=None, marker_normal_noisy=None)
            with Recorder() as rec:
                out = fn(batch)
            key = '{}/call{}/'.format(name, call)
            got = [(k, v.numpy()) for k, v in rec.calls]
            if kind == 'spherical':
                assert [k for k, _ in got] == ['randperm', 'randint', 'rand', 'rand', 'rand']
                data[key + 'sensor'] = got[0][1][:kw['num_markers']].astype(np.int32)
                data[key + 'start'] = got[1][1].astype(np.int32)
                data[key + 'u_r'] = got[2][1]
                # (the reference's own expressions on the recorded uniform draws)
                data[key + 'theta'] = (torch.from_numpy(got[3][1]) * np.pi * 2).numpy()
                data[key + 'phi'] = (torch.from_numpy(got[4][1]) * np.pi).numpy()
                data[key + 'max_r'] = np.asarray(fn.max_r, np.float64)
                assert out.marker_ori_noisy is None and out.marker_normal_noisy is None
            else:
                assert [k for k, _ in got] == ['randint', 'randint']
                data[key + 'sensor'] = fn.marker_ids.cpu().numpy()[got[0][1]].astype(np.int32)
                data[key + 'start'] = got[1][1].astype(np.int32)
                data[key + 'mask_value'] = np.asarray(fn.mask_value, np.float64)
                data[key + 'ori_out'] = out.marker_ori_noisy.numpy()
                data[key + 'normal_out'] = out.marker_normal_noisy.numpy()
            data[key + 'window_len'] = np.asarray(int(fn.ws * F), np.int32)
            data[key + 'pos_out'] = out.marker_pos_noisy.numpy()
    np.savez_compressed(OUT, **data)
    print('wrote', OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
