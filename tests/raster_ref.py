"""
NumPy restatement of the rasteriser's definition (include/empose_hip.h, csrc/raster.hip), operation by operation, in a
chosen dtype: float64 is what the HIP kernels are held to, float32 is the control that shows what the number format
alone costs.  Also the scenes that tests/test_render_cpu.py (their conditions, on the CPU) and tests/test_render.py (the
kernels, on the GPU) share.

The inputs are float32 numbers (vertices, camera, intrinsics: what the kernels are handed); only the arithmetic changes
with `dtype`.

Besides the images, `raster_frame` returns the AMBIGUITY MASK of the frame, always from float64 arithmetic: a pixel is
ambiguous when
  (i)  its centre lies within EDGE_TOL pixels of an edge line of a face for which at most one edge function is negative
       there (the centre is on, or just outside, that face's outline), or
  (ii) the second-nearest face covering it is within DEPTH_TOL relative depth of the nearest.
At such a pixel float32 may pick another face than float64 without being wrong; everywhere else it may not.
"""
import collections

import numpy as np

EDGE_TOL = 1e-3      # pixels
DEPTH_TOL = 1e-4     # relative
WAVE_PIXELS = 256    # csrc/raster_kernels.h RASTER_WAVE_PIXELS: larger bounding boxes take the kernel's wave path

Frame = collections.namedtuple('Frame', 'face_id depth rgb ambiguous normal_ok covered n_small n_large n_near_dropped')


def _f32(x, dtype):
    return np.asarray(np.asarray(x, dtype=np.float32), dtype=dtype)


def project(vertices, R, t, fx, fy, cx, cy, dtype):
    p, R, t = _f32(vertices, dtype), _f32(R, dtype), _f32(t, dtype)
    fx, fy, cx, cy = (_f32(v, dtype) for v in (fx, fy, cx, cy))
    cam = [((R[r, 0] * p[:, 0] + R[r, 1] * p[:, 1]) + R[r, 2] * p[:, 2]) + t[r] for r in range(3)]
    with np.errstate(all='ignore'):
        return np.stack([(fx * cam[0]) / cam[2] + cx, (fy * cam[1]) / cam[2] + cy, cam[2]], axis=1)


def _edges(tri, px, py, flip):
    (x0, y0), (x1, y1), (x2, y2) = tri
    w0 = (x2 - x1) * (py - y1) - (y2 - y1) * (px - x1)
    w1 = (x0 - x2) * (py - y2) - (y0 - y2) * (px - x2)
    w2 = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)
    return (-w0, -w1, -w2) if flip else (w0, w1, w2)


def _box(xs, ys, H, W, dtype, grow=0):
    half = dtype(0.5)
    jl = max(np.ceil(min(xs) - half) - grow, 0.0)
    jh = min(np.floor(max(xs) - half) + grow, float(W - 1))
    il = max(np.ceil(min(ys) - half) - grow, 0.0)
    ih = min(np.floor(max(ys) - half) + grow, float(H - 1))
    if not (jl <= jh and il <= ih):
        return None
    return int(il), int(ih), int(jl), int(jh)


def _raster(proj, faces, near, H, W, dtype, ambiguity):
    """-> nearest face id, its depth, the second-nearest depth, the edge-ambiguity mask (float64 only), counters."""
    near = _f32(near, dtype)
    half = dtype(0.5)
    f1 = np.full((H, W), -1, dtype=np.int32)
    z1 = np.full((H, W), np.inf, dtype=dtype)
    z2 = np.full((H, W), np.inf, dtype=dtype)
    amb = np.zeros((H, W), dtype=bool)
    n_small = n_large = n_dropped = 0
    for f, (a, b, c) in enumerate(faces):
        (x0, y0, Z0), (x1, y1, Z1), (x2, y2, Z2) = proj[a], proj[b], proj[c]
        zs = (Z0, Z1, Z2)
        if not all(z > near for z in zs):
            n_dropped += any(z > near for z in zs)     # (a face that CROSSES the plane)
            continue
        area = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0)
        if area == 0:
            continue
        tri = ((x0, y0), (x1, y1), (x2, y2))
        box = _box((x0, x1, x2), (y0, y1, y2), H, W, dtype)
        if box is not None:
            i0, i1, j0, j1 = box
            if (i1 - i0 + 1) * (j1 - j0 + 1) > WAVE_PIXELS:
                n_large += 1
            else:
                n_small += 1
            py = (np.arange(i0, i1 + 1).astype(dtype) + half)[:, None]
            px = (np.arange(j0, j1 + 1).astype(dtype) + half)[None, :]
            w0, w1, w2 = _edges(tri, px, py, area < 0)
            ws = (w0 + w1) + w2
            cov = (w0 >= 0) & (w1 >= 0) & (w2 >= 0) & (ws > 0)
            if cov.any():
                with np.errstate(all='ignore'):
                    Z = ws / ((w0 / Z0 + w1 / Z1) + w2 / Z2)
                s1, s2, sf = z1[i0:i1 + 1, j0:j1 + 1], z2[i0:i1 + 1, j0:j1 + 1], f1[i0:i1 + 1, j0:j1 + 1]
                wins = cov & (Z < s1)            # faces come in ascending order: on a tie the lower id stays
                second = cov & ~wins & (Z < s2)
                s2[wins] = s1[wins]
                s1[wins] = Z[wins]
                sf[wins] = f
                s2[second] = Z[second]
        if ambiguity:
            box = _box((x0, x1, x2), (y0, y1, y2), H, W, dtype, grow=1)
            if box is None:
                continue
            i0, i1, j0, j1 = box
            py = (np.arange(i0, i1 + 1).astype(dtype) + half)[:, None]
            px = (np.arange(j0, j1 + 1).astype(dtype) + half)[None, :]
            w = _edges(tri, px, py, area < 0)
            lens = (np.hypot(x2 - x1, y2 - y1), np.hypot(x0 - x2, y0 - y2), np.hypot(x1 - x0, y1 - y0))
            close = np.zeros(w[0].shape, dtype=bool)
            for wk, lk in zip(w, lens):
                if lk > 0:
                    close |= np.abs(wk) < EDGE_TOL * lk
                else:
                    close |= True      # two corners coincide: everything about this face is ambiguous nearby
            n_neg = (w[0] < 0).astype(int) + (w[1] < 0) + (w[2] < 0)
            amb[i0:i1 + 1, j0:j1 + 1] |= close & (n_neg <= 1)
    return f1, z1, z2, amb, n_small, n_large, n_dropped


def raster_frame(vertices, faces, R, t, fx, fy, cx, cy, near, H, W, dtype=np.float64, normals=None, colors=(0.7, 0.7, 0.7),
                 light=(0.0, 0.0, -1.0), ambient=0.3, background=(1.0, 1.0, 1.0), variants=None):
    """One frame.  vertices (V, 3), faces (F, 3) int, normals None (flat) or (V, 3), colors (3,) or (V, 3).
    `variants` ({name: {'normals': ..., 'colors': ...}}): several shadings of the one visibility; `rgb` and `normal_ok` of
    the result are then dicts by name."""
    dtype = np.dtype(dtype).type
    faces = np.asarray(faces).astype(np.int64)
    proj = project(vertices, R, t, fx, fy, cx, cy, dtype)
    # the mask comes from float64 whatever the dtype of the images
    if dtype is np.float64:
        f1, z1, y2, amb, n_small, n_large, n_dropped = _raster(proj, faces, near, H, W, dtype, True)
        g1, y1 = f1, z1
    else:
        f1, z1, _, _, n_small, n_large, n_dropped = _raster(proj, faces, near, H, W, dtype, False)
        p64 = project(vertices, R, t, fx, fy, cx, cy, np.float64)
        g1, y1, y2, amb, _, _, _ = _raster(p64, faces, near, H, W, np.float64, True)
    with np.errstate(invalid='ignore'):
        amb |= (g1 >= 0) & ((y2 - y1) <= DEPTH_TOL * y1)

    # shading, as raster_shade_kernel: barycentrics recomputed at the winning face
    half = dtype(0.5)
    ii, jj = np.nonzero(f1 >= 0)
    fa = faces[f1[ii, jj]]
    px, py = jj.astype(dtype) + half, ii.astype(dtype) + half
    P = [proj[fa[:, k]] for k in range(3)]
    area = (P[1][:, 0] - P[0][:, 0]) * (P[2][:, 1] - P[0][:, 1]) - (P[1][:, 1] - P[0][:, 1]) * (P[2][:, 0] - P[0][:, 0])
    w = _edges(tuple((p[:, 0], p[:, 1]) for p in P), px, py, False)
    sign = np.where(area < 0, dtype(-1), dtype(1))
    w = [wk * sign for wk in w]
    ws = (w[0] + w[1]) + w[2]
    lam = [wk / ws for wk in w]
    v = _f32(vertices, dtype)

    def shade(normals, colors):
        if normals is not None:
            nv = _f32(normals, dtype)
            n = (lam[0][:, None] * nv[fa[:, 0]] + lam[1][:, None] * nv[fa[:, 1]]) + lam[2][:, None] * nv[fa[:, 2]]
        else:
            e1, e2 = v[fa[:, 1]] - v[fa[:, 0]], v[fa[:, 2]] - v[fa[:, 0]]
            n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                          e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        Rd = _f32(R, dtype)
        nc = np.stack([(Rd[r, 0] * n[:, 0] + Rd[r, 1] * n[:, 1]) + Rd[r, 2] * n[:, 2] for r in range(3)], axis=1)
        length = np.sqrt((nc[:, 0] * nc[:, 0] + nc[:, 1] * nc[:, 1]) + nc[:, 2] * nc[:, 2])
        l64 = np.asarray(light, dtype=np.float64)
        l = _f32(l64 / np.linalg.norm(l64), dtype)     # normalised in double on the host, handed over as float32
        dot = (nc[:, 0] * l[0] + nc[:, 1] * l[1]) + nc[:, 2] * l[2]
        amb_l = _f32(ambient, dtype)
        with np.errstate(all='ignore'):
            inten = np.where(length > 0, amb_l + (dtype(1) - amb_l) * (np.abs(dot) / length), amb_l)
        col = _f32(colors, dtype)
        if col.ndim == 1:
            base = np.broadcast_to(col, (len(ii), 3))
        else:
            base = (lam[0][:, None] * col[fa[:, 0]] + lam[1][:, None] * col[fa[:, 1]]) + lam[2][:, None] * col[fa[:, 2]]
        to_byte = lambda c: np.floor(np.clip(dtype(255) * c + half, 0, 255)).astype(np.uint8)
        rgb = np.empty((H, W, 3), dtype=np.uint8)
        rgb[:] = to_byte(_f32(background, dtype))
        rgb[ii, jj] = to_byte(base * inten[:, None])
        normal_ok = np.ones((H, W), dtype=bool)
        if len(ii):
            normal_ok[ii, jj] = length > 1e-6 * length.max()
        return rgb, normal_ok

    if variants is None:
        rgb, normal_ok = shade(normals, colors)
    else:       # the visibility once, every shading of the list on top of it
        shaded = {name: shade(kw.get('normals'), kw.get('colors', colors)) for name, kw in variants.items()}
        rgb, normal_ok = {k: v[0] for k, v in shaded.items()}, {k: v[1] for k, v in shaded.items()}
    return Frame(f1, z1, rgb, amb, normal_ok, f1 >= 0, n_small, n_large, n_dropped)


# ---- the scenes ---------------------------------------------------------------------------------------------------------
# Bodies of the synthetic model (synthetic.make_model) with perturbed shape, root rotation and pose.  fx = fy = 1.1 W and
# the principal point at the image centre unless a scene moves it.
Scene = collections.namedtuple('Scene', 'name nu nv T H W eyes target cx_shift near seed cap')
EYE, TARGET = (0.6, 0.3, 2.6), (0.0, -0.2, 0.0)
SMALL_CAP, FULL_CAP = 0.02, 0.10       # ambiguous pixels over covered pixels, at most
SCENES = [
    Scene('one_frame', 10, 16, 1, 48, 64, [EYE], TARGET, 0.0, 0.05, 11, SMALL_CAP),
    Scene('three_frames', 10, 16, 3, 97, 131, [EYE], TARGET, 0.0, 0.05, 12, SMALL_CAP),
    Scene('leaves_image', 10, 16, 1, 48, 64, [EYE], TARGET, 0.3, 0.05, 13, SMALL_CAP),
    Scene('crosses_near', 10, 16, 1, 97, 131, [(0.15, 0.0, 0.62)], TARGET, 0.0, 0.5, 14, SMALL_CAP),
    Scene('camera_per_frame', 10, 16, 3, 48, 64, [EYE, (-0.9, 0.5, 2.4), (1.6, -0.1, 2.0)], TARGET, 0.0, 0.05, 15,
          SMALL_CAP),
    Scene('full_mesh', 65, 106, 1, 120, 160, [EYE], TARGET, 0.0, 0.05, 16, FULL_CAP),
]


def scene_inputs(scene):
    """poses_root (T, 3), poses_body (T, 63), betas (T, 10), float32."""
    rng = np.random.default_rng(scene.seed)
    return (rng.normal(0.0, 0.3, size=(scene.T, 3)).astype(np.float32),
            rng.normal(0.0, 0.15, size=(scene.T, 63)).astype(np.float32),
            rng.normal(0.0, 1.0, size=(scene.T, 10)).astype(np.float32))


def scene_camera(scene):
    """A vis.camera.Camera with float32-exact numbers: R (3, 3) / t (3,), or (T, 3, 3) / (T, 3) for a camera per frame."""
    from em_pose_amd.vis.camera import Camera, look_at
    Rt = [look_at(e, scene.target) for e in scene.eyes]
    R = np.stack([r for r, _ in Rt]).astype(np.float32)
    t = np.stack([x for _, x in Rt]).astype(np.float32)
    if len(scene.eyes) == 1:
        R, t = R[0], t[0]
    f32 = lambda x: float(np.float32(x))
    return Camera(R, t, f32(1.1 * scene.W), f32(1.1 * scene.W), f32(scene.W / 2.0 + scene.cx_shift * scene.W),
                  f32(scene.H / 2.0), f32(scene.near))


def reference_frames(scene, vertices, faces, dtype=np.float64, **shading):
    """`raster_frame` per frame of a scene; `normals` / `colors` in `shading` may carry a leading frame axis."""
    cam = scene_camera(scene)
    out = []
    for k in range(scene.T):
        R, t = (cam.R[k], cam.t[k]) if cam.R.ndim == 3 else (cam.R, cam.t)
        per_frame = lambda d: {key: (v[k] if key in ('normals', 'colors') and v is not None and np.ndim(v) == 3 else v)
                               for key, v in d.items()}
        sh = per_frame(shading)
        if sh.get('variants') is not None:
            sh['variants'] = {name: per_frame(kw) for name, kw in sh['variants'].items()}
        out.append(raster_frame(vertices[k], faces, R, t, cam.fx, cam.fy, cam.cx, cam.cy, cam.near, scene.H, scene.W,
                                dtype=dtype, **sh))
    return out
