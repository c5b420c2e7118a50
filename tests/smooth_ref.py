"""Float64 NumPy restatement of the two pose filters that csrc/smooth.hip defines (include/empose_hip.h, DESIGN.md section
9), written from the formulas as host code, and the input generator of their tests.  It shares no code with the package;
the quaternion helpers are those of tests/resample_ref.py ((w, x, y, z) rows).

A row is [3 J rotation-vector columns | C linear columns | anything].  A frame counts where `valid` is set (None: every
frame); a run is a maximal stretch of consecutive counting frames of one row.  Both functions return float64 rows of
3 J + C columns; a frame that does not count keeps its input there (the tests compare those frames by their bits).
`stats`, when given, is a list that receives every aligned quaternion dot product the restatement forms (|<c, q>|): the
definitions are discontinuous where one is 0.

  window64    for a counting frame t of the run [a, b]: r = min(R, t - a, b - t);
              channel:  acc = w0 x[t]; k = 1 .. r ascending: acc += w_k (x[t-k] + x[t+k]), wsum += 2 w_k; out = acc / wsum
              rotation: c = q(r[t]); acc = w0 c; acc += w_k (s- q(r[t-k]) + s+ q(r[t+k])), s = -1 where <c, q> < 0 else +1;
                        out = rotation vector of acc / |acc| with w >= 0
              (the loop over k runs over all frames at once, each frame taking part while k <= its r: per frame it is the
              sequence of operations above, in that order)
  one_euro64  alpha(fc) = 1 / (1 + fps / (2 pi fc)); first counting frame of a run: x^ = x, s^ = 0; afterwards
              channel:  d = (x - x^) fps; s^ += alpha(d_cutoff) (d - s^); fc = min_cutoff + beta |s^|; x^ += alpha(fc) (x - x^)
              rotation: q in the hemisphere of x^; delta = log(x^-1 q); theta = 2 |delta|; d = theta fps; s^, fc as above;
                        x^ <- x^ exp(alpha(fc) delta) / |.|; out = its rotation vector with w >= 0
              a frame that does not count ends the run and clears the state; frame after frame, in order.
"""
import numpy as np

from tests import resample_ref as Q
from tests import temporal_ref as T

STATE = 6   # x^ (4; a channel uses the first) | s^ | live


def _valid(valid, n, f):
    return np.ones((n, f), dtype=bool) if valid is None else np.asarray(valid).reshape(n, f) != 0


def half_widths(valid, R):
    """(n, f) int: r = min(R, t - a, b - t) at the counting frames of the runs [a, b], -1 at the others."""
    n, f = valid.shape
    r = np.full((n, f), -1, dtype=np.int64)
    for i in range(n):
        t = 0
        while t < f:
            if not valid[i, t]:
                t += 1
                continue
            a = t
            while t + 1 < f and valid[i, t + 1]:
                t += 1
            b = t
            for u in range(a, b + 1):
                r[i, u] = min(R, u - a, b - u)
            t += 1
    return r


def window64(rows, valid, taps, J, C, stats=None):
    x = np.asarray(rows, dtype=np.float64)
    n, f = x.shape[:2]
    v = _valid(valid, n, f)
    w = np.asarray(taps, dtype=np.float64)
    R = w.shape[0] - 1
    r = half_widths(v, R)
    out = x[..., :3 * J + C].copy()
    with np.errstate(invalid='ignore', over='ignore'):   # a frame that does not count may hold anything
        q = Q.quat_from_rotvec(x[..., :3 * J].reshape(n, f, J, 3))   # (n, f, J, 4)
        lin = x[..., 3 * J:3 * J + C]
    acc_q = np.where(v[:, :, None, None], w[0] * q, 0.0)
    acc_l = np.where(v[:, :, None], w[0] * lin, 0.0)
    wsum = np.full((n, f), w[0])
    for k in range(1, R + 1):
        i, t = np.nonzero(r >= k)       # the frames whose window reaches k; t - k and t + k are inside their run
        if i.size == 0:
            break
        c, p, s = q[i, t], q[i, t - k], q[i, t + k]
        dp, ds = (c * p).sum(axis=-1, keepdims=True), (c * s).sum(axis=-1, keepdims=True)
        if stats is not None and J:
            stats.append(float(min(np.abs(dp).min(), np.abs(ds).min())))
        sp, ss = np.where(dp < 0, -1.0, 1.0), np.where(ds < 0, -1.0, 1.0)
        acc_q[i, t] = acc_q[i, t] + w[k] * (sp * p + ss * s)
        acc_l[i, t] = acc_l[i, t] + w[k] * (lin[i, t - k] + lin[i, t + k])
        wsum[i, t] = wsum[i, t] + 2.0 * w[k]
    i, t = np.nonzero(v)
    if i.size:
        a = acc_q[i, t]
        out[i, t, :3 * J] = Q.quat_to_rotvec(a / np.linalg.norm(a, axis=-1, keepdims=True)).reshape(i.size, 3 * J)
        out[i, t, 3 * J:] = acc_l[i, t] / wsum[i, t][:, None]
    return out


def alpha(fps, fc):
    return 1.0 / (1.0 + fps / (2.0 * np.pi * fc))


def one_euro64(rows, valid, J, C, fps, min_cutoff, beta, d_cutoff, state=None, stats=None):
    """-> (out (n, f, 3 J + C), state (n, J + C, 6)).  `state`: what an earlier call returned (None: every row starts fresh)."""
    x = np.asarray(rows, dtype=np.float64)
    n, f = x.shape[:2]
    v = _valid(valid, n, f)
    out = x[..., :3 * J + C].copy()
    st = np.zeros((n, J + C, STATE)) if state is None else np.array(state, dtype=np.float64)
    a_d = alpha(fps, d_cutoff)
    for i in range(n):
        xq, xl = st[i, :J, :4].copy(), st[i, J:, 0].copy()
        sq, sl = st[i, :J, 4].copy(), st[i, J:, 4].copy()
        live = bool(st[i, 0, 5] != 0.0)
        for t in range(f):
            if not v[i, t]:
                live = False
                xq[:], xl[:], sq[:], sl[:] = 0.0, 0.0, 0.0, 0.0
                continue
            q = Q.quat_from_rotvec(x[i, t, :3 * J].reshape(J, 3))
            lin = x[i, t, 3 * J:3 * J + C]
            if not live:
                xq, xl = q.copy(), lin.copy()
                sq[:], sl[:] = 0.0, 0.0
                live = True
            else:
                dot = (xq * q).sum(axis=-1, keepdims=True)
                if stats is not None and J:
                    stats.append(float(np.abs(dot).min()))
                q = np.where(dot < 0, -q, q)
                delta = Q.quat_log(Q.quat_mul(Q.quat_inv(xq), q))
                theta = 2.0 * np.linalg.norm(delta, axis=-1)
                d = theta * fps
                sq = sq + a_d * (d - sq)
                fc = min_cutoff + beta * np.abs(sq)
                y = Q.quat_mul(xq, Q.quat_exp(alpha(fps, fc)[:, None] * delta))
                xq = y / np.linalg.norm(y, axis=-1, keepdims=True)
                d = (lin - xl) * fps
                sl = sl + a_d * (d - sl)
                fc = min_cutoff + beta * np.abs(sl)
                xl = xl + alpha(fps, fc) * (lin - xl)
            out[i, t, :3 * J] = Q.quat_to_rotvec(xq).reshape(3 * J)
            out[i, t, 3 * J:] = xl
        st[i] = 0.0
        if live:
            st[i, :J, :4], st[i, J:, 0] = xq, xl
            st[i, :J, 4], st[i, J:, 4] = sq, sl
            st[i, :, 5] = 1.0
    return out, st


# ---- comparison ------------------------------------------------------------------------------------------------------------
ROT_TOL = 1e-6   # rad, ROT_TOL of tests/test_resample.py: fp32 rounding of a rotation vector of length <= pi moves it by
                 # at most 2^-24 pi sqrt 3 = 3.3e-7 rad, times three


def linear_bound(want, x_max):
    """|got - want| allowed on a linear channel: both sides are float64 on identical inputs, so fewer than 5000 roundings at
    the magnitude of the inputs (1e-12 max|x|), plus the one fp32 ulp by which two nearly equal doubles can round apart."""
    return np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 1e-12 * x_max


def worst_ratios(got, want, rows, valid, J, C):
    """The largest error / tolerance over the counting frames of (rotations by geodesic angle, linear channels), and
    whether the frames that do not count are bit copies of the input.  got: float32 (n, f, >= 3 J + C)."""
    n, f = got.shape[:2]
    v = _valid(valid, n, f)
    rot = lin = 0.0
    if J and v.any():
        ang = Q.geodesic(got[v][:, :3 * J].astype(np.float64).reshape(-1, J, 3), want[v][:, :3 * J].reshape(-1, J, 3))
        rot = float(ang.max()) / ROT_TOL
        assert float(np.linalg.norm(got[v][:, :3 * J].reshape(-1, 3), axis=-1).max()) <= np.pi * (1 + 2.0 ** -22)
    if C and v.any():
        w = want[v][:, 3 * J:3 * J + C]
        x_max = float(np.abs(np.asarray(rows)[v][:, 3 * J:3 * J + C]).max())
        lin = float((np.abs(got[v][:, 3 * J:3 * J + C].astype(np.float64) - w) / linear_bound(w, x_max)).max())
    cols = 3 * J + C
    copies = np.array_equal(np.ascontiguousarray(got[~v][:, :cols]).view(np.uint32),
                            np.ascontiguousarray(np.asarray(rows, dtype=np.float32)[~v][:, :cols]).view(np.uint32))
    return rot, lin, copies


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def rotation_walk(rng, f, start, axis0=None):
    """(f, 4) unit quaternions: from `start`, a step of 0.04 rad per frame about a drifting axis (from `axis0`, or a random
    one), then 0.02 rad of independent noise on every frame."""
    axis = rng.normal(size=3) if axis0 is None else np.array(axis0, dtype=np.float64)
    axis /= np.linalg.norm(axis)
    cur = np.array(start, dtype=np.float64)
    out = np.empty((f, 4))
    for t in range(f):
        if t:
            axis = axis + 0.05 * rng.normal(size=3)
            axis /= np.linalg.norm(axis)
            cur = Q.quat_mul(cur, Q.quat_exp(0.02 * axis))        # half-angle vector: 0.04 rad
        noise = rng.normal(size=3)
        noise *= 0.01 / np.linalg.norm(noise)                     # 0.02 rad about a random axis
        out[t] = Q.quat_mul(cur, Q.quat_exp(noise))
    return out


def make_rows(rng, n, f, J, C, ld=None, ragged=True):
    """-> rows (n, f, ld) float32, valid (n, f) bool.  Joint j of row i with (i + j) even starts at angle pi - 0.6 and turns
    on about its own axis, so it passes through |r| = pi after about 15 frames; near there some of its inputs are given as
    the equivalent rotation vector of length above pi.  The others start anywhere.  Linear channels: a slow sinusoid plus
    noise, magnitude below 2.  Validity as temporal_ref.ragged_valid, with row 1 dead when there are three rows; the frames
    that do not count, and the padding, hold NaN."""
    cols = 3 * J + C
    ld = cols if ld is None else ld
    rows = np.full((n, f, ld), np.nan, dtype=np.float32)
    for i in range(n):
        for j in range(J):
            if (i + j) % 2 == 0:
                u = rng.normal(size=3)
                u /= np.linalg.norm(u)
                q = rotation_walk(rng, f, Q.quat_exp(0.5 * (np.pi - 0.6) * u), axis0=u)
            else:
                q = rotation_walk(rng, f, Q.quat_exp(rng.normal(size=3)))
            r = Q.quat_to_rotvec(q)
            ang = np.linalg.norm(r, axis=-1, keepdims=True)
            longer = (ang[:, 0] > 2.5) & (rng.uniform(size=f) < 0.3)
            r[longer] = (r * (1.0 - 2.0 * np.pi / np.where(ang > 0, ang, 1.0)))[longer]   # the same rotation, |r| = 2 pi - angle > pi
            rows[i, :, 3 * j:3 * j + 3] = r
        t = np.arange(f)[:, None]
        rows[i, :, 3 * J:cols] = 1.7 * np.sin(2 * np.pi * rng.uniform(0.2, 2.0, size=(1, C)) * t / 60.0 +
                                              rng.uniform(0, 2 * np.pi, size=(1, C))) + rng.normal(0, 0.05, size=(f, C))
    valid = T.ragged_valid(rng, n, f, dead_row=1 if n >= 3 else None) if ragged else np.ones((n, f), dtype=bool)
    rows[~valid, :cols] = np.nan
    return rows, valid


JC = ((1, 0), (0, 1), (22, 10), (24, 13))
RADII = (0, 1, 2, 8, 32)


def frames(S):
    return (1, 2, 3, S - 1, S, S + 1, 2 * S + 33)


_CASES = {}


def case(n, f, J, C):
    """The inputs of one test shape (tight rows), made once and left unchanged."""
    key = (n, f, J, C)
    if key not in _CASES:
        rows, valid = make_rows(np.random.default_rng([n, f, J, C]), n, f, J, C)
        rows.setflags(write=False)
        valid.setflags(write=False)
        _CASES[key] = (rows, valid)
    return _CASES[key]


_WINDOWS = {}


def window_case(n, f, J, C, R, sigma=None):
    """The window restatement of a shape with Gaussian taps of sigma = max(R, 1) / 2 frames, computed once."""
    key = (n, f, J, C, R)
    if key not in _WINDOWS:
        rows, valid = case(n, f, J, C)
        k = np.arange(R + 1, dtype=np.float64)
        taps = np.exp(-(k * k) / (2.0 * (0.5 * max(R, 1)) ** 2))
        want = window64(rows, valid, taps, J, C)
        want.setflags(write=False)
        _WINDOWS[key] = (taps, want)
    return _WINDOWS[key]
