"""The write step of the sensor-noise augmentation (reference data/noise_functions.py:98-106,156-163) restated in float64
NumPy for a given plan, the fixture recorded from the reference (tests/golden/sensor_noise.npz), and the plumbing that
hands a plan to `empose_sensor_noise`.  A helper, not a test."""
import ctypes as C
import os

import numpy as np
import torch

from em_pose_amd import _lib

SPHERICAL, SUPPRESS = 0, 1
THIGH = (5, 6)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sensor_noise.npz')
CASES = ('spherical_a', 'spherical_b', 'suppress_a', 'suppress_b')


def load_fixture():
    """{'pos', 'ori', 'normal', 'thigh_idx', cases: {name: [call0, call1]}}, every call a plan plus the reference's
    outputs."""
    z = np.load(GOLDEN)
    fx = {k: z[k] for k in ('pos', 'ori', 'normal', 'thigh_idx')}
    fx['cases'] = {}
    for k in z.files:
        if '/' in k:
            name, call, field = k.split('/')
            fx['cases'].setdefault(name, [{}, {}])[int(call[-1])][field] = z[k]
    return fx


def plan_of(call):
    """A recorded call as the keyword arguments of `restate` / `run_kernel`."""
    if 'u_r' in call:
        return dict(mode=SPHERICAL, start=call['start'], sensor=call['sensor'], window_len=int(call['window_len']),
                    u_r=call['u_r'], theta=call['theta'], phi=call['phi'], max_r=float(call['max_r']))
    return dict(mode=SUPPRESS, start=call['start'], sensor=call['sensor'], window_len=int(call['window_len']),
                mask_value=float(call['mask_value']))


def affected(n, f, m, start, sensor, window_len, mode):
    """(n, f, m) bool: the sensors the plan touches."""
    hit = np.zeros((n, f, m), bool)
    for i in range(n):
        ids = np.asarray(sensor[i] if mode == SUPPRESS else sensor).reshape(-1)
        hit[i, int(start[i]):int(start[i]) + window_len, ids] = True
    return hit


def restate(pos, ori=None, normal=None, *, mode, start, sensor, window_len, u_r=None, theta=None, phi=None, max_r=0.0,
            mask_value=0.0, thigh=THIGH):
    """float64 outputs (pos, ori, normal); spherical: (pos, None, None).  Untouched elements are the inputs' values."""
    n, f = pos.shape[:2]
    m = pos.shape[2] // 3
    if mode == SUPPRESS:
        hit = affected(n, f, m, start, sensor, window_len, mode)
        outs = []
        for x, c in ((pos, 3), (ori, 9), (normal, 3)):
            o = x.astype(np.float64).reshape(n, f, m, c)
            o[hit] = mask_value
            outs.append(o.reshape(n, f, m * c))
        return tuple(outs)
    p = pos.astype(np.float64).reshape(n, f, m, 3)
    out = p.copy()
    thigh_len = np.linalg.norm(p[0, f // 2, thigh[0]] - p[0, 0, thigh[1]])
    r = u_r.astype(np.float64) * max_r * thigh_len / 2
    th, ph = theta.astype(np.float64), phi.astype(np.float64)
    d = np.stack([r * np.cos(th) * np.sin(ph), r * np.sin(th) * np.cos(ph), r * np.cos(ph)], -1)   # (n, wl, K, 3)
    for i in range(n):
        s = int(start[i])
        for k, sid in enumerate(np.asarray(sensor).reshape(-1)):   # a sensor named twice: its last entry counts
            out[i, s:s + window_len, int(sid)] = p[i, s:s + window_len, int(sid)] + d[i, :, k]
    return out.reshape(n, f, m * 3), None, None


def check_against_reference(fx, call, got):
    """`got` (pos, ori, normal) against what the reference wrote for the recorded call: suppression and every element the
    plan does not touch exactly, displaced positions within 1e-6.  Returns the largest error of a displaced position."""
    plan = plan_of(call)
    n, f = fx['pos'].shape[:2]
    m = fx['pos'].shape[2] // 3
    hit = affected(n, f, m, plan['start'], plan['sensor'], plan['window_len'], plan['mode'])
    if plan['mode'] == SUPPRESS:
        for g, name in zip(got, ('pos_out', 'ori_out', 'normal_out')):
            assert np.array_equal(np.asarray(g, np.float64), call[name].astype(np.float64)), name
        return 0.0
    assert got[1] is None and got[2] is None
    g = np.asarray(got[0], np.float64).reshape(n, f, m, 3)
    want = call['pos_out'].astype(np.float64).reshape(n, f, m, 3)
    assert np.array_equal(g[~hit], want[~hit]) and np.array_equal(g[~hit], fx['pos'].reshape(n, f, m, 3)[~hit])
    err = float(np.abs(g[hit] - want[hit]).max()) if hit.any() else 0.0
    assert err <= 1e-6, err
    return err


def call_abi(mode, n, f, m, k, window_len, start_host, sensor_host, start_dev, sensor_dev, u_r, theta, phi, max_r, thigh_a,
             thigh_b, mask_value, pos, ori, normal, pos_out, ori_out, normal_out, stream=None):
    """The raw entry point: every pointer a c_void_p or None."""
    return _lib.lib().empose_sensor_noise(mode, n, f, m, k, window_len, start_host, sensor_host, start_dev, sensor_dev,
                                          u_r, theta, phi, max_r, thigh_a, thigh_b, mask_value, pos, ori, normal,
                                          pos_out, ori_out, normal_out, stream)


def run_kernel(pos, ori=None, normal=None, *, mode, start, sensor, window_len, u_r=None, theta=None, phi=None, max_r=0.0,
               mask_value=0.0, thigh=THIGH, device='cuda:0'):
    """The kernel on host arrays: float32 numpy outputs (pos, ori, normal); spherical: (pos, None, None)."""
    n, f = pos.shape[:2]
    m = pos.shape[2] // 3
    start = np.ascontiguousarray(start, np.int32)
    sensor = np.ascontiguousarray(sensor, np.int32)
    k = sensor.shape[-1]
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)
    d_in = [up(pos), up(ori), up(normal)] if mode == SUPPRESS else [up(pos), None, None]
    d_out = [None if x is None else torch.empty_like(x) for x in d_in]
    d_plan = [up(start), up(sensor)]
    d_draw = [up(None if a is None else np.asarray(a, np.float32)) for a in (u_r, theta, phi)]
    ptr = lambda t: None if t is None or t.numel() == 0 else _lib.dptr(t)
    with torch.cuda.device(device):
        _lib.check(call_abi(mode, n, f, m, k, window_len, C.c_void_p(start.ctypes.data), C.c_void_p(sensor.ctypes.data),
                            ptr(d_plan[0]), ptr(d_plan[1]), ptr(d_draw[0]), ptr(d_draw[1]), ptr(d_draw[2]), max_r,
                            thigh[0], thigh[1], mask_value, ptr(d_in[0]), ptr(d_in[1]), ptr(d_in[2]), ptr(d_out[0]),
                            ptr(d_out[1]), ptr(d_out[2]), _lib.current_stream()))
    return tuple(None if x is None else x.cpu().numpy() for x in d_out)
