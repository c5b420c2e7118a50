"""Float64 NumPy restatement of the temporal metrics, written from their definitions, frame by frame:
for one sequence of points x[t] at `fps` frames per second, with backward stencils,
  acc[t]  = (x[t] - 2 x[t-1] + x[t-2]) fps^2               defined where frames t-2 .. t all count
  jerk[t] = (x[t] - 3 x[t-1] + 3 x[t-2] - x[t-3]) fps^3    defined where frames t-3 .. t all count
and per (frame, point) |acc_gt - acc_hat|, |jerk_hat|, |jerk_gt|.  A stencil never reaches across a frame that does not
count, and never across two rows.  What the tests of empose_temporal_rows and TemporalMetricsEngine compare against."""
import numpy as np

from em_pose_amd.eval.metrics import EUCL_EVAL_JOINTS
from em_pose_amd.helpers.configuration import CONSTANTS as C

ACC, JERK = 1, 2   # bits of `defined`


def rows64(x_gt, x_hat, valid, fps):
    """x_gt, x_hat (n, f, P, 3), valid (n, f) -> rows (n, f, 3 P) float64 = |acc_gt - acc_hat| | |jerk_hat| | |jerk_gt|
    (0 where undefined) and defined (n, f) uint8."""
    g, h = np.asarray(x_gt, dtype=np.float64), np.asarray(x_hat, dtype=np.float64)
    v = np.asarray(valid) != 0
    n, f, P = g.shape[:3]
    fps = float(fps)
    rows = np.zeros((n, f, 3 * P))
    defined = np.zeros((n, f), dtype=np.uint8)
    for i in range(n):
        for t in range(f):
            if t >= 2 and v[i, t] and v[i, t - 1] and v[i, t - 2]:
                acc_g = (g[i, t] - 2.0 * g[i, t - 1] + g[i, t - 2]) * fps ** 2
                acc_h = (h[i, t] - 2.0 * h[i, t - 1] + h[i, t - 2]) * fps ** 2
                rows[i, t, :P] = np.linalg.norm(acc_g - acc_h, axis=-1)
                defined[i, t] |= ACC
            if t >= 3 and v[i, t] and v[i, t - 1] and v[i, t - 2] and v[i, t - 3]:
                jerk_g = (g[i, t] - 3.0 * g[i, t - 1] + 3.0 * g[i, t - 2] - g[i, t - 3]) * fps ** 3
                jerk_h = (h[i, t] - 3.0 * h[i, t - 1] + 3.0 * h[i, t - 2] - h[i, t - 3]) * fps ** 3
                rows[i, t, P:2 * P] = np.linalg.norm(jerk_h, axis=-1)
                rows[i, t, 2 * P:] = np.linalg.norm(jerk_g, axis=-1)
                defined[i, t] |= JERK
    return rows, defined


def reduced64(rows):
    """Per-point rows (n, f, 3 P) -> (n, f, 6): per quantity the sum over the P points and the sum of squares."""
    n, f = rows.shape[:2]
    q = rows.reshape(n, f, 3, -1)
    return np.stack([q.sum(axis=-1), (q * q).sum(axis=-1)], axis=-1).reshape(n, f, 6)


def families(rows, defined):
    """The rows the engine accumulates, batch row after batch row, frames in order:
    {'accel' (m_a, P), 'jitter' (m_j, P), 'jitter_gt' (m_j, P)}."""
    P = rows.shape[-1] // 3
    acc, jerk = (defined & ACC) != 0, (defined & JERK) != 0
    return {'accel': rows[acc][:, :P], 'jitter': rows[jerk][:, P:2 * P], 'jitter_gt': rows[jerk][:, 2 * P:]}


def joint_columns(fam, select=True):
    """The joint columns by the conventions of MPJPE: the mean over frames per joint, then over EUCL_EVAL_JOINTS; the STD
    over all selected (frame, joint) entries.  NaN for a family without a frame."""
    out = {}
    for key, name in (('accel', 'Accel'), ('jitter', 'Jitter'), ('jitter_gt', 'Jitter GT')):
        unit = ' [m/s^2]' if key == 'accel' else ' [m/s^3]'
        a = fam[key]
        if a.shape[0] == 0:
            out[name + unit] = out[name + ' STD'] = float('nan')
            continue
        idx = [C.SMPL_JOINTS.index(j) for j in EUCL_EVAL_JOINTS] if select else list(range(a.shape[1]))
        out[name + unit] = float(np.mean([a[:, j].mean() for j in idx]))
        out[name + ' STD'] = float(np.std(a[:, idx]))
    return out


def smooth_points(rng, n, f, P, fps=60.0, noise=1e-3):
    """Smooth test trajectories: per point and axis a sum of three sinusoids of amplitude <= 0.5 m and 0.5 - 3 Hz sampled at
    `fps`; the estimate is the truth plus float32 noise of `noise` metres.  -> x_gt, x_hat (n, f, P, 3) float32."""
    t = np.arange(f, dtype=np.float64)[None, :, None, None, None] / fps
    amp = rng.uniform(0.0, 0.5 / 3.0, size=(n, 1, P, 3, 3))
    hz = rng.uniform(0.5, 3.0, size=(n, 1, P, 3, 3))
    ph = rng.uniform(0.0, 2.0 * np.pi, size=(n, 1, P, 3, 3))
    x = (amp * np.sin(2.0 * np.pi * hz * t + ph)).sum(axis=-1).astype(np.float32)
    x_hat = (x + rng.normal(0.0, noise, size=x.shape).astype(np.float32)).astype(np.float32)
    return x, x_hat


def ragged_valid(rng, n, f, rate=0.03, dead_row=None):
    """(n, f) bool: frames invalid at `rate`, and optionally one row without a single counting frame."""
    v = rng.uniform(size=(n, f)) >= rate
    if dead_row is not None:
        v[dead_row] = False
    return v
