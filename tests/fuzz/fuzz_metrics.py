"""Randomized checks of the device metrics kernel (`empose_metrics_rows`, csrc/metrics.hip) against a float64 reference
written from the maths: NumPy's LAPACK SVD for the Procrustes alignment, the clamped Rodrigues map of the reference
(helpers/so3.py:116-121) for the global joint orientations.  Besides well-conditioned bodies the generator draws the
frames where a 3 x 3 SVD goes wrong: near-planar / planar / collinear point sets, repeated singular values, mirror
images, large offsets, and the angle edges (0, 180 degrees, below the exp-map clamp).

    python tests/fuzz/fuzz_metrics.py <seed> <seconds | n=CASES>

`run()` is shared with tests/test_metrics_kernel.py (a fixed-seed slice inside `pytest -m gpu`).  The inputs are
float32 (what the kernel takes); the reference evaluates the SAME float32 values in float64, so every difference is the
kernel's own arithmetic.  The bounds are absolute and the same for every family (TOL)."""
import sys
import time

if __name__ == '__main__':
    sys.path.insert(0, '.')

import numpy as np

from em_pose_amd.helpers.configuration import CONSTANTS as C

NJ = 22
PARENTS = tuple(C.SMPL_PARENTS[:NJ])
TOL = {'eucl': 1e-12, 'pa': 1e-8, 'angle': 1e-5}       # metres, metres, degrees
COLUMNS = {'eucl': slice(0, 22), 'pa': slice(22, 44), 'angle': slice(44, 65)}
CLAMP_SQ = 1e-4                                       # exp map: angle clamped at 1e-2 rad (so3.py:116-121)

FAMILIES = ('well_conditioned', 'smpl_bodies', 'near_planar_gt', 'planar_gt', 'near_planar_hat', 'planar_hat',
            'collinear_hat', 'repeated_singular_values', 'identical', 'mirror', 'large_offsets', 'angle_zero',
            'angle_near_180', 'angle_below_clamp', 'no_poses', 'coincident_gt', 'coincident_hat')
# families whose PA columns are NaN by definition (a point set without spread cannot be normalised)
NAN_PA = ('coincident_gt', 'coincident_hat')


# ---- float64 reference -----------------------------------------------------------------------------------------------
def exp_map_clamped(r):
    """(..., 3) axis-angle -> (..., 3, 3), float64: R = I + sin(a)/a K + (1 - cos a)/a^2 K^2 with a = sqrt(max(|r|^2,
    1e-4)) -- the reference's clamped Rodrigues (below 1e-2 rad not exactly a rotation, on purpose)."""
    r = np.asarray(r, dtype=np.float64)
    a = np.sqrt(np.maximum((r * r).sum(-1), CLAMP_SQ))[..., None, None]
    K = np.zeros(r.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 2] = -r[..., 2], r[..., 1], -r[..., 0]
    K[..., 1, 0], K[..., 2, 0], K[..., 2, 1] = r[..., 2], -r[..., 1], r[..., 0]
    return np.eye(3) + np.sin(a) / a * K + (1.0 - np.cos(a)) / (a * a) * (K @ K)


def global_orientations(pose, parents=PARENTS, rodrigues=exp_map_clamped):
    """pose (T, 63) body axis-angles (joints 1..21) -> global orientations (T, 22, 3, 3), root = identity."""
    pose = np.asarray(pose, dtype=np.float64).reshape(-1, NJ - 1, 3)
    local = rodrigues(pose)
    G = np.empty((pose.shape[0], NJ, 3, 3))
    G[:, 0] = np.eye(3)
    for j in range(1, NJ):
        G[:, j] = G[:, parents[j]] @ local[:, j - 1]
    return G


def procrustes_distances(X, Y):
    """Per-joint distances |X - (s R Y + t)| after the optimal similarity alignment of Y onto X (rotation, not a
    reflection): X, Y (T, J, 3) float64.  SVD of X0^T Y0 from LAPACK; a frame whose X or Y has no spread is NaN."""
    muX, muY = X.mean(1, keepdims=True), Y.mean(1, keepdims=True)
    X0, Y0 = X - muX, Y - muY
    nX = np.sqrt((X0 ** 2).sum((1, 2)))
    nY = np.sqrt((Y0 ** 2).sum((1, 2)))
    out = np.full(X.shape[:2], np.nan)
    ok = (nX > 0) & (nY > 0)
    if not ok.any():
        return out
    X0, Y0, nX, nY, muX = X0[ok] / nX[ok, None, None], Y0[ok] / nY[ok, None, None], nX[ok], nY[ok], muX[ok]
    U, s, Vt = np.linalg.svd(np.swapaxes(X0, 1, 2) @ Y0)
    V = np.swapaxes(Vt, 1, 2)
    d = np.sign(np.linalg.det(V @ np.swapaxes(U, 1, 2)))     # +-1: V and U are orthogonal
    V[:, :, 2] *= d[:, None]
    s[:, 2] *= d
    T = V @ np.swapaxes(U, 1, 2)
    Z = nX[:, None, None] * s.sum(1)[:, None, None] * (Y0 @ T) + muX
    out[ok] = np.sqrt(((X[ok] - Z) ** 2).sum(-1))
    return out


def reference_rows(joints_gt, joints_hat, pose_gt=None, pose_hat=None, parents=PARENTS):
    """What one row of empose_metrics_rows should hold, in float64: (T, 65) = 22 Euclidean distances | 22 distances
    after Procrustes | 21 geodesic angles (degrees) between the global orientations of joints 1..21 (0 without poses)."""
    X = np.asarray(joints_gt, dtype=np.float64).reshape(-1, NJ, 3)
    Y = np.asarray(joints_hat, dtype=np.float64).reshape(-1, NJ, 3)
    rows = np.zeros((X.shape[0], 65))
    rows[:, :22] = np.sqrt(((X - Y) ** 2).sum(-1))
    rows[:, 22:44] = procrustes_distances(X, Y)
    if pose_gt is not None:
        Gg, Gh = global_orientations(pose_gt, parents)[:, 1:], global_orientations(pose_hat, parents)[:, 1:]
        c = np.clip(((Gg * Gh).sum((-1, -2)) - 1.0) * 0.5, -1.0, 1.0)
        rows[:, 44:] = np.degrees(np.arccos(c))
    return rows


# ---- case generators -------------------------------------------------------------------------------------------------
def random_rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def similarity(rng, P, noise=0.05):
    """s R P + t + noise, per frame (P (T, J, 3) float64)."""
    out = np.empty_like(P)
    for t in range(P.shape[0]):
        out[t] = rng.uniform(0.5, 2.0) * P[t] @ random_rotation(rng).T + rng.normal(0, 0.5, size=3)
    return out + rng.normal(0, noise, size=P.shape)


def body_cloud(rng, T, spread=0.3):
    return rng.normal(0, spread, size=(T, NJ, 3)) + rng.normal(0, 1.0, size=(T, 1, 3))


def planar_cloud(rng, T, eps, rotate, spread=0.3):
    """Points spread over a plane with thickness eps; `rotate`: a random orientation (its float32 rounding then adds
    ~1e-8 of thickness), else the plane z = 0 itself (thickness exactly eps in float32)."""
    P = rng.normal(0, spread, size=(T, NJ, 3))
    P[..., 2] = eps * rng.uniform(-1, 1, size=(T, NJ))
    if rotate:
        for t in range(T):
            P[t] = P[t] @ random_rotation(rng).T
        P += rng.normal(0, 1.0, size=(T, 1, 3))
    else:
        P[..., :2] += rng.normal(0, 1.0, size=(T, 1, 2))
    return P


def symmetric_cloud(rng, T):
    """Point sets whose scatter matrix has a repeated eigenvalue: octahedra (three equal singular values) or square
    prisms (two equal) at several scales, the remaining joints at the centre (which is the centroid)."""
    octa = np.concatenate([np.eye(3), -np.eye(3)])
    prism = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-0.5, 0.5)], dtype=np.float64)
    out = np.zeros((T, NJ, 3))
    for t in range(T):
        pts = np.concatenate([octa, 0.5 * octa, 0.25 * octa]) if rng.integers(0, 2) else \
            np.concatenate([prism, 0.5 * prism])
        out[t, :pts.shape[0]] = 0.2 * pts @ (random_rotation(rng).T if rng.integers(0, 2) else np.eye(3))
    return out


_BM = None


def smpl_joints(pose, shape, root):
    """SMPL forward kinematics of the small test model (oracle/torch_ref.py, float64): joints (T, 22, 3)."""
    global _BM
    import torch
    from oracle import torch_ref as R
    if _BM is None:
        from tests.helpers import small_model
        _BM = R.BodyModelTensors(small_model(), dtype=torch.float64)
    _, j = R.smpl_fk(_BM, torch.from_numpy(pose), torch.from_numpy(shape), torch.from_numpy(root))
    return j[:, :NJ].numpy()


def random_poses(rng, T, scale=0.3):
    return rng.normal(0, scale, size=(T, 63))


def _angle_near_180(rng, T):
    """Every joint under a root child is turned by pi - delta relative to the ground truth: the child of the root turns
    about a shared axis, its descendants keep the same local rotations (so their relative rotation is conjugate)."""
    pg = random_poses(rng, T)
    ph = pg.copy()
    for t in range(T):
        delta = float(rng.choice([0.0, 1e-7, 1e-6, 1e-4, 1e-2, 0.1]))
        for j in (1, 2, 3):                       # children of the root: pose entries (j - 1) * 3
            n = rng.normal(size=3)
            n /= np.linalg.norm(n)
            a = rng.uniform(-1.0, 1.0)
            pg[t, (j - 1) * 3:j * 3] = a * n
            ph[t, (j - 1) * 3:j * 3] = (a - (np.pi - delta)) * n
    return pg, ph


def _angle_below_clamp(rng, T):
    """Local rotations shorter than the 1e-2 rad clamp.  Half the frames turn every joint about ONE axis, the ground
    truth by +|r| and the estimate by -|r| with |r| = 1e-2 / sqrt(3): along the seven-joint chain to a wrist, the
    clamp's deviation from the exact map adds up to ~5e-5 degrees -- more than TOL['angle'], so a kernel without the
    clamp fails this family."""
    pg, ph = rng.normal(0, 3e-3, size=(T, 63)), rng.normal(0, 3e-3, size=(T, 63))
    for t in range(0, T, 2):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        r = 1e-2 / np.sqrt(3.0) * n
        pg[t] = np.tile(r, NJ - 1)
        ph[t] = -pg[t]
    return pg, ph


def make_case(family, rng, T):
    """One case of a family: (joints_gt, joints_hat, pose_gt, pose_hat), float32 (poses None for 'no_poses')."""
    pg = random_poses(rng, T)
    ph = pg + rng.normal(0, 0.2, size=pg.shape)
    if family == 'well_conditioned':
        X = body_cloud(rng, T)
        Y = similarity(rng, X) if rng.integers(0, 2) else X + rng.normal(0, 0.05, size=X.shape)
    elif family == 'smpl_bodies':
        shape = rng.normal(0, 1, size=(T, 10))
        X = smpl_joints(pg, shape, rng.normal(0, 0.5, size=(T, 3)))
        Y = smpl_joints(ph, shape + rng.normal(0, 0.3, size=shape.shape), rng.normal(0, 0.5, size=(T, 3)))
        Y += rng.normal(0, 0.3, size=(T, 1, 3))
    elif family in ('near_planar_gt', 'planar_gt'):
        eps = 0.0 if family == 'planar_gt' else float(rng.choice([1e-1, 1e-3, 1e-6, 1e-8, 1e-9, 1e-10, 1e-11, 1e-12]))
        X = planar_cloud(rng, T, eps, rotate=bool(rng.integers(0, 2)))
        Y = similarity(rng, X)
    elif family in ('near_planar_hat', 'planar_hat', 'collinear_hat'):
        X = body_cloud(rng, T)
        if family == 'collinear_hat':
            d = rng.normal(size=(T, 1, 3))
            Y = rng.normal(0, 0.3, size=(T, NJ, 1)) * d + rng.normal(0, 1.0, size=(T, 1, 3))
        else:
            eps = 0.0 if family == 'planar_hat' else float(rng.choice([1e-1, 1e-3, 1e-6, 1e-8, 1e-10, 1e-12]))
            Y = planar_cloud(rng, T, eps, rotate=bool(rng.integers(0, 2)))
    elif family == 'repeated_singular_values':
        X = symmetric_cloud(rng, T)
        Y = X.copy() if rng.integers(0, 2) else similarity(rng, X, noise=0.0)
    elif family == 'identical':
        X = body_cloud(rng, T)
        Y = X.copy()
    elif family == 'mirror':
        X = body_cloud(rng, T) if rng.integers(0, 2) else smpl_joints(pg, rng.normal(0, 1, size=(T, 10)),
                                                                       rng.normal(0, 0.5, size=(T, 3)))
        Y = X * np.array([1.0, 1.0, -1.0])
    elif family == 'large_offsets':
        X = body_cloud(rng, T) + rng.uniform(-8, 8, size=(T, 1, 3))
        Y = X + rng.normal(0, 0.05, size=X.shape) + rng.normal(0, 0.1, size=(T, 1, 3))
    elif family == 'angle_zero':
        X = body_cloud(rng, T)
        Y = X + rng.normal(0, 0.05, size=X.shape)
        ph = pg.copy()
        pg[::2] *= 1e-3                                    # (below the clamp as well)
        ph[::2] = pg[::2]
    elif family == 'angle_near_180':
        X = body_cloud(rng, T)
        Y = X + rng.normal(0, 0.05, size=X.shape)
        pg, ph = _angle_near_180(rng, T)
    elif family == 'angle_below_clamp':
        X = body_cloud(rng, T)
        Y = X + rng.normal(0, 0.05, size=X.shape)
        pg, ph = _angle_below_clamp(rng, T)
    elif family == 'no_poses':
        X = body_cloud(rng, T)
        Y = similarity(rng, X)
        pg = ph = None
    elif family in ('coincident_gt', 'coincident_hat'):
        X, Y = body_cloud(rng, T), body_cloud(rng, T)
        P = X if family == 'coincident_gt' else Y
        P[:] = P[:, :1]
    else:
        raise ValueError(family)
    f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)
    return f32(X), f32(Y), f32(pg), f32(ph)


def case_errors(got, want, family):
    """Worst absolute difference per column group; NaN where the two disagree on being NaN (inf: a failure)."""
    err = {}
    for key, cols in COLUMNS.items():
        g, w = got[:, cols], want[:, cols]
        if key == 'pa' and family in NAN_PA:
            err[key] = 0.0 if (np.isnan(g).all() and np.isnan(w).all()) else np.inf
            continue
        if not (np.isfinite(g).all() and np.isfinite(w).all()):
            err[key] = np.inf
            continue
        err[key] = float(np.abs(g - w).max()) if g.size else 0.0
    return err


# ---- device ----------------------------------------------------------------------------------------------------------
def device_rows(X, Y, pg=None, ph=None, parents=PARENTS, extra_rows=0, fill=np.nan):
    """empose_metrics_rows on cuda:0; returns the (T + extra_rows, 65) block (rows past T pre-filled with `fill`)."""
    import ctypes
    import torch
    from em_pose_amd import _lib
    T = X.shape[0]
    dev = torch.device('cuda:0')
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    x, y, g, h = up(X), up(Y), up(pg), up(ph)
    rows = torch.full((T + extra_rows, 65), fill, dtype=torch.float64, device=dev)
    par = (ctypes.c_int * NJ)(*parents)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().empose_metrics_rows(T, _lib.dptr(x), _lib.dptr(y), _lib.dptr(g), _lib.dptr(h), par,
                                                  _lib.dptr(rows), _lib.current_stream()))
    torch.cuda.synchronize(dev)
    return rows.cpu().numpy()


def run(seed=0, seconds=None, n_cases=None, families=FAMILIES, log=print, max_frames=96, check=True):
    """Cases round-robin over `families` (so a slice of n cases visits every family n / len(families) times), T frames
    per case drawn from 1..max_frames.  Returns {'n', 'worst': {family: {column group: error}}, 'worst_case': {family:
    case}, 'failures': [(case, family, errors)]}; with `check` the first failure raises."""
    rng = np.random.default_rng(seed)
    t_end = time.time() + (seconds if seconds is not None else 1e9)
    worst = {f: {k: 0.0 for k in COLUMNS} for f in families}
    worst_case = {f: None for f in families}
    failures, n = [], 0
    while time.time() < t_end and (n_cases is None or n < n_cases):
        family = families[n % len(families)]
        T = int(rng.integers(1, max_frames + 1))
        X, Y, pg, ph = make_case(family, rng, T)
        got = device_rows(X, Y, pg, ph)
        err = case_errors(got, reference_rows(X, Y, pg, ph), family)
        for k, e in err.items():
            if not e <= worst[family][k]:
                worst[family][k] = e
                worst_case[family] = n
        bad = {k: e for k, e in err.items() if not e <= TOL[k]}
        if bad:
            failures.append((n, family, err))
            log('metrics case %d (%s, T=%d) out of bounds: %s' % (n, family, T, bad))
            assert not check, 'METRICS MISMATCH seed %d case %d %s: %r' % (seed, n, family, err)
        n += 1
    return {'n': n, 'worst': worst, 'worst_case': worst_case, 'failures': failures}


def report(r):
    lines = ['%d cases; worst abs error per family (bounds: eucl %.0e m, pa %.0e m, angle %.0e deg):'
             % (r['n'], TOL['eucl'], TOL['pa'], TOL['angle'])]
    for f, e in r['worst'].items():
        lines.append('  %-26s eucl %.2e  pa %.2e  angle %.2e  (case %s)' % (f, e['eucl'], e['pa'], e['angle'],
                                                                          r['worst_case'][f]))
    lines.append('%d cases out of bounds' % len(r['failures']))
    return '\n'.join(lines)


if __name__ == '__main__':
    arg = sys.argv[2] if len(sys.argv) > 2 else '60'
    r = run(int(sys.argv[1]) if len(sys.argv) > 1 else 0, n_cases=int(arg[2:]) if arg.startswith('n=') else None,
            seconds=None if arg.startswith('n=') else float(arg), check=False)
    print(report(r))
    sys.exit(1 if r['failures'] else 0)
