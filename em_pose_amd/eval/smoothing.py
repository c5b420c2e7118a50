"""
Smoothing of estimated pose sequences: what reduces the trembling that `TemporalMetricsEngine` measures.  The frame-wise
models and the sensor fit with a weak smoothness prior put frame-independent noise on the pose; two filters take it off,
both in HIP (`empose_smooth_window`, `empose_smooth_one_euro`, csrc/smooth.hip: fp32 in and out, float64 arithmetic):

  `smooth_window`   for whole recordings: a zero-phase symmetric FIR window (`gaussian_taps`).  At the ends of a run of
                    counting frames the window shrinks symmetrically, so it never leaves the run, constant-velocity motion
                    is reproduced and the end frames pass through.
  `OneEuroFilter`   for streaming (what `net(chunk, is_new_sequence=False)` exists for): the causal One-Euro filter of
                    Casiez, Roussel and Vogel (CHI 2012), a first-order low-pass whose cut-off rises with the speed.  The
                    defaults are the paper's (`min_cutoff` 1 Hz, `beta` 0, `d_cutoff` 1 Hz); no tuning for EM data is claimed.

A row is `[3 * n_joints rotation-vector columns | n_channels linear columns]`.  Rotations are filtered as rotations, on
SO(3) through unit quaternions -- the window as the sign-aligned chordal mean, this project's definition -- and never as
rotation-vector components, which jump at |r| = pi; every rotation vector that comes out has |r| <= pi.  A frame that
does not count (`valid`) is copied bit for bit, ends the run, and what it holds never reaches another frame.  The exact
definitions stand in include/empose_hip.h and DESIGN.md section 9.

`smooth_model_output` filters root orientation, body pose and shape of a model's output and recomputes the joints from
the filtered pose by forward kinematics -- never filtered joints, which would not belong to any pose: the rule
`ResampleSequence` follows.

Device tensors only: CPU tensors raise, as the layer does.
"""
import ctypes
import math

import numpy as np
import torch

from em_pose_amd import _lib
from em_pose_amd.helpers.configuration import CONSTANTS as C

MAX_RADIUS = _lib.SMOOTH_MAX_RADIUS


def gaussian_taps(sigma_frames, radius=None):
    """One side w[0 .. radius] of a Gaussian kernel, w[k] = exp(-k^2 / (2 sigma^2)) (float64; the filter divides by the
    sum of the taps it uses).  `radius` defaults to min(32, ceil(3 sigma))."""
    sigma = float(sigma_frames)
    if not (sigma > 0.0 and math.isfinite(sigma)):
        raise ValueError('sigma_frames must be positive and finite')
    if radius is None:
        radius = min(MAX_RADIUS, int(math.ceil(3.0 * sigma)))
    radius = int(radius)
    if not 0 <= radius <= MAX_RADIUS:
        raise ValueError('radius must be in [0, {}]'.format(MAX_RADIUS))
    k = np.arange(radius + 1, dtype=np.float64)
    return np.exp(-(k * k) / (2.0 * sigma * sigma))


def _rows(rows, valid, n_joints, n_channels):
    """The checked arguments of both filters: (n, f, rows as float32 with unit column stride, valid uint8 or None)."""
    if not rows.is_cuda:
        raise _lib.EmposeError('the smoothing filters need GPU tensors (got device {}); there is no CPU fallback'
                               .format(rows.device))
    if rows.dim() != 3:
        raise ValueError('rows must be (n, f, columns)')
    n, f, cols = int(rows.shape[0]), int(rows.shape[1]), int(rows.shape[2])
    if cols < 3 * int(n_joints) + int(n_channels):
        raise ValueError('rows of {} columns cannot hold {} joints and {} channels'.format(cols, n_joints, n_channels))
    rows = rows.detach().to(torch.float32).contiguous()
    if valid is not None:
        valid = (valid.reshape(n, f).to(rows.device) != 0).to(torch.uint8).contiguous()
    return n, f, rows, valid


def smooth_window(rows, valid, taps, n_joints, n_channels):
    """`empose_smooth_window`: rows (n, f, >= 3 * n_joints + n_channels) on the device, valid (n, f) or None (every frame
    counts), taps = w[0 .. R] (host floats, e.g. `gaussian_taps`).  -> the filtered rows, float32, same shape; columns
    beyond the filtered ones are copied.  Nothing waits for the device."""
    n, f, rows, valid = _rows(rows, valid, n_joints, n_channels)
    taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).reshape(-1))
    out = rows.clone()
    with torch.cuda.device(rows.device):
        _lib.check(_lib.lib().empose_smooth_window(
            n, f, int(n_joints), int(n_channels), _lib.dptr(rows), rows.shape[2], _lib.dptr(valid), taps.shape[0] - 1,
            taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _lib.dptr(out), out.shape[2], _lib.current_stream()))
    return out


class OneEuroFilter(object):
    def __init__(self, n_joints, n_channels, fps=C.FPS, min_cutoff=1.0, beta=0.0, d_cutoff=1.0):
        """The defaults are those of the original paper; `fps` is the project's frame rate."""
        for name, v in (('fps', fps), ('min_cutoff', min_cutoff), ('d_cutoff', d_cutoff)):
            if not (float(v) > 0.0 and math.isfinite(float(v))):
                raise ValueError('{} must be positive and finite'.format(name))
        if not (float(beta) >= 0.0 and math.isfinite(float(beta))):
            raise ValueError('beta must be finite and not negative')
        if int(n_joints) < 0 or int(n_channels) < 0 or int(n_joints) + int(n_channels) == 0:
            raise ValueError('n_joints and n_channels must not be negative, and one must be positive')
        self.n_joints, self.n_channels = int(n_joints), int(n_channels)
        self.fps, self.min_cutoff, self.beta, self.d_cutoff = float(fps), float(min_cutoff), float(beta), float(d_cutoff)
        self.reset()

    def reset(self):
        """Forget the carried state: the next call must start new sequences."""
        self._state = None   # (n, n_joints + n_channels, 6) float64 on the device

    def __call__(self, rows, valid=None, is_new_sequence=True):
        """rows (n, f, >= 3 * n_joints + n_channels) on the device, valid (n, f) or None.  `is_new_sequence` has the
        meaning it has in `net(chunk, is_new_sequence=)` and in `TemporalMetricsEngine`: with False, batch row i continues
        row i of the previous call, and the rows that go on are the first k.  -> the filtered rows, float32."""
        n, f, rows, valid = _rows(rows, valid, self.n_joints, self.n_channels)
        state_in = None
        if not is_new_sequence:
            if self._state is None:
                raise ValueError('is_new_sequence=False, but there is no previous call to continue')
            if self._state.device != rows.device:
                raise ValueError('is_new_sequence=False on another device than the previous call')
            if n > self._state.shape[0]:
                raise ValueError('is_new_sequence=False with {} rows, the previous call had {}: the rows that go on are '
                                 'the first k'.format(n, self._state.shape[0]))
            state_in = self._state[:n].contiguous()
        state_out = torch.empty(n, self.n_joints + self.n_channels, _lib.SMOOTH_STATE, dtype=torch.float64,
                                device=rows.device)
        out = rows.clone()
        with torch.cuda.device(rows.device):
            _lib.check(_lib.lib().empose_smooth_one_euro(
                n, f, self.n_joints, self.n_channels, _lib.dptr(rows), rows.shape[2], _lib.dptr(valid), self.fps,
                self.min_cutoff, self.beta, self.d_cutoff, _lib.dptr(state_in), _lib.dptr(state_out), _lib.dptr(out),
                out.shape[2], _lib.current_stream()))
        self._state = state_out
        return out


def window_filter(taps):
    """A `filt` for `smooth_model_output`: the window with these taps."""
    return lambda rows, valid, n_joints, n_channels: smooth_window(rows, valid, taps, n_joints, n_channels)


def smooth_model_output(model_out, valid, smpl_model, filt, is_new_sequence=True):
    """Filters a model's estimate: packs `root_ori_hat | pose_hat | shape_hat` of `model_out` (each (n, f, .)) into rows of
    22 joints and as many channels as there are betas, filters them, and returns a new dict with the filtered three and
    `joints_hat` from `smpl_model.fk_joints` of the filtered pose and shape ((n, f, 66), as the models give it).  The
    other entries are passed on.  `filt`: a `OneEuroFilter(22, n_betas)` (its state is carried with
    `is_new_sequence=False`), or a callable (rows, valid, n_joints, n_channels) -> rows such as `window_filter(taps)`.
    valid (n, f) or None."""
    root, pose, shape = model_out['root_ori_hat'], model_out['pose_hat'], model_out['shape_hat']
    if not (root.is_cuda and pose.is_cuda and shape.is_cuda):
        raise _lib.EmposeError('smooth_model_output needs GPU tensors; there is no CPU fallback')
    n, f = int(pose.shape[0]), int(pose.shape[1])
    nb = C.N_JOINTS * 3
    if shape.dim() == 2:
        shape = shape.unsqueeze(1).expand(n, f, shape.shape[-1])
    n_betas = int(shape.shape[-1])
    n_joints = C.N_JOINTS + 1
    rows = torch.cat([root.reshape(n, f, 3), pose[..., :nb], shape], dim=-1).to(torch.float32)
    if isinstance(filt, OneEuroFilter):
        if (filt.n_joints, filt.n_channels) != (n_joints, n_betas):
            raise ValueError('the filter is for {} joints and {} channels, the estimate has {} and {}'.format(
                filt.n_joints, filt.n_channels, n_joints, n_betas))
        rows = filt(rows, valid, is_new_sequence=is_new_sequence)
    else:
        rows = filt(rows, valid, n_joints, n_betas)
    out = dict(model_out)
    out['root_ori_hat'] = rows[..., :3].contiguous()
    out['pose_hat'] = rows[..., 3:3 + nb].contiguous()
    out['shape_hat'] = rows[..., 3 + nb:].contiguous()
    flat = lambda t: t.reshape(n * f, -1)
    out['joints_hat'] = smpl_model.fk_joints(flat(out['pose_hat']), flat(out['shape_hat']),
                                             poses_root=flat(out['root_ori_hat'])).reshape(n, f, -1)
    return out
