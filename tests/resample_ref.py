"""Float64 NumPy restatement of the rotation resampling that csrc/resample.hip defines (the oracle of
tests/test_resample.py), written from the formulas as sequential host code: the global `fix_quaternions` pass along
time, explicit phantom knots at both ends, a control point at every knot, then one output frame after the other.  It
shares no code with the package.  Quaternions are (w, x, y, z) rows."""
import numpy as np


def quat_from_rotvec(r):
    r = np.asarray(r, dtype=np.float64)
    angle = np.linalg.norm(r, axis=-1, keepdims=True)
    half = 0.5 * angle
    k = np.where(angle < 1e-12, 0.5, np.sin(half) / np.where(angle < 1e-12, 1.0, angle))
    return np.concatenate([np.cos(half), k * r], axis=-1)


def quat_to_rotvec(q):
    """The rotation vector with w >= 0, |r| <= pi."""
    q = np.where(q[..., :1] < 0, -q, q)
    s = np.linalg.norm(q[..., 1:], axis=-1, keepdims=True)
    k = np.where(s < 1e-12, 2.0, 2.0 * np.arctan2(s, q[..., :1]) / np.where(s < 1e-12, 1.0, s))
    return k * q[..., 1:]


def quat_mul(a, b):
    aw, ax, ay, az = np.moveaxis(a, -1, 0)
    bw, bx, by, bz = np.moveaxis(b, -1, 0)
    return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=-1)


def quat_inv(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def quat_log(q):
    """Pure-quaternion logarithm of a unit quaternion as a 3-vector (half the rotation vector)."""
    s = np.linalg.norm(q[..., 1:], axis=-1, keepdims=True)
    k = np.where(s < 1e-12, 1.0, np.arctan2(s, q[..., :1]) / np.where(s < 1e-12, 1.0, s))
    return k * q[..., 1:]


def quat_exp(v):
    a = np.linalg.norm(v, axis=-1, keepdims=True)
    k = np.where(a < 1e-12, 1.0, np.sin(a) / np.where(a < 1e-12, 1.0, a))
    return np.concatenate([np.cos(a), k * v], axis=-1)


def slerp(a, b, t):
    return quat_mul(a, quat_exp(t * quat_log(quat_mul(quat_inv(a), b))))


def fix_quaternions(q):
    """Sequential pass along time (axis 0): every quaternion into the hemisphere of its (already fixed) predecessor."""
    q = q.copy()
    for k in range(1, q.shape[0]):
        flip = np.sum(q[k - 1] * q[k], axis=-1, keepdims=True) < 0
        q[k] = np.where(flip, -q[k], q[k])
    return q


def n_frames_out(n_frames, fps_in, fps_out):
    return len(np.arange(0, n_frames / fps_in, 1 / fps_out))


def resample_rotations(rotations, fps_in, fps_out):
    """(F, N, 3) rotation vectors (any float type; computed in float64) -> (F', N, 3) float64."""
    rotations = np.asarray(rotations, dtype=np.float64)
    n = rotations.shape[0]
    assert n > 1
    q = fix_quaternions(quat_from_rotvec(rotations))                       # (F, N, 4)
    before = quat_mul(quat_mul(q[0], quat_inv(q[1])), q[0])                # phantom knots, constant velocity
    after = quat_mul(quat_mul(q[n - 1], quat_inv(q[n - 2])), q[n - 1])
    ext = np.concatenate([before[None], q, after[None]], axis=0)           # ext[k + 1] = q_k
    ctrl = np.empty_like(q)
    for k in range(n):
        prev, cur, nxt = ext[k], ext[k + 1], ext[k + 2]
        ctrl[k] = quat_mul(cur, quat_exp(0.25 * (quat_log(quat_mul(quat_inv(prev), cur)) -
                                                 quat_log(quat_mul(quat_inv(cur), nxt)))))
    out = np.empty((n_frames_out(n, fps_in, fps_out),) + rotations.shape[1:])
    for k in range(out.shape[0]):
        u = (k / fps_out) * fps_in
        i = min(int(np.floor(u)), n - 2)
        tau = u - i
        res = slerp(slerp(q[i], q[i + 1], tau), slerp(ctrl[i], ctrl[i + 1], tau), 2.0 * tau * (1.0 - tau))
        out[k] = quat_to_rotvec(res)
    return out


def rotmat(r):
    """(..., 3) rotation vectors -> (..., 3, 3), float64."""
    q = quat_from_rotvec(r)
    w, x, y, z = np.moveaxis(q, -1, 0)
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], -1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], -1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1)], -2)


def geodesic(r_a, r_b):
    """Angle (rad) between the rotations of two arrays of rotation vectors, through float64 rotation matrices: atan2 of
    the antisymmetric and the trace part of R_a^T R_b, accurate near 0."""
    rel = np.swapaxes(rotmat(r_a), -1, -2) @ rotmat(r_b)
    w = np.stack([rel[..., 2, 1] - rel[..., 1, 2], rel[..., 0, 2] - rel[..., 2, 0], rel[..., 1, 0] - rel[..., 0, 1]], -1)
    return np.arctan2(0.5 * np.linalg.norm(w, axis=-1), 0.5 * (np.trace(rel, axis1=-2, axis2=-1) - 1.0))
