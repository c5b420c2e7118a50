"""
Numpy restatement of the two definitions behind `em_pose_amd.eval.surface_metrics`, written from the
definitions and not from the kernel: the closest point of a triangle mesh to a query, and the parity test for "inside".
Both run in the dtype they are given (`closest_point(..., dtype=np.float32)` is the float32 run the tolerance comes from);
the inside test is always float64, as the kernel's is.  Also the meshes and the query sets the tests share.
"""
import numpy as np

from em_pose_amd.synthetic import torus_grid_faces

# Largest |float32 run - float64 run| of this restatement over the queries of `gpu_cases()` (coordinates within 2 m):
# 1.52e-7 m in `dist`, 1.68e-7 m in `closest` -- the float64 closest point on the face the float32 run chose: at a point
# with two nearest faces the choice is legitimately not unique -- (tests/test_surface_query_cpu.py measures both again),
# times the margin of 4 for the kernel's operation order and fused multiply-adds, 6.74e-7, rounded up.  A query further out
# than 2 m is allowed the same in proportion: `tolerance(points)`.
TOL_MARGIN = 4.0
TOL_M = 7e-7


def tolerance(points):
    """Per query: TOL_M, scaled by max |coordinate| / 2 m beyond 2 m (the 100 m query)."""
    p = np.asarray(points, dtype=np.float64)
    return TOL_M * np.maximum(1.0, np.abs(p).max(axis=-1) / 2.0)


# ---- closest point -----------------------------------------------------------------------------------------------------
def _dot(u, v):
    return u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1] + u[..., 2] * v[..., 2]


def closest_pairs(p, a, b, c):
    """The closest point of every triangle (a, b, c) to every p, arrays that broadcast to (..., 3), in their own dtype:
    Voronoi regions in the order vertex a, vertex b, edge ab, vertex c, edge ac, edge bc, interior, every comparison
    inclusive, a quotient with a denominator that is not positive taken as 0.  Returns (d2, point, bary)."""
    dt = np.result_type(p, a)
    zero, one = dt.type(0), dt.type(1)
    ab, ac = b - a, c - a
    ap, bp, cp = p - a, p - b, p - c
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4

    def quot(num, den):
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(den > 0, num / np.where(den > 0, den, one), zero).astype(dt)
    t_ab = quot(d1, d1 - d3)
    t_ac = quot(d2, d2 - d6)
    t_bc = quot(d4 - d3, (d4 - d3) + (d5 - d6))
    pa, pb, pc = np.maximum(va, zero), np.maximum(vb, zero), np.maximum(vc, zero)
    s = (pa + pb) + pc
    v_in, w_in = quot(pb, s), quot(pc, s)
    regions = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
               (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & ((d4 - d3) >= 0) & ((d5 - d6) >= 0)]
    shape = regions[0].shape
    z, o = np.zeros(shape, dt), np.ones(shape, dt)
    barys = [(o, z, z), (z, o, z), (one - t_ab, t_ab, z), (z, z, o), (one - t_ac, z, t_ac), (z, one - t_bc, t_bc)]
    full = lambda x: np.broadcast_to(x, shape + (3,))
    points = [full(a), full(b), a + t_ab[..., None] * ab, full(c), a + t_ac[..., None] * ac, b + t_bc[..., None] * (c - b)]
    bary = np.stack([np.maximum((one - v_in) - w_in, zero), v_in, w_in], axis=-1)
    point = (a + v_in[..., None] * ab) + w_in[..., None] * ac
    taken = np.zeros(shape, bool)
    for region, (u, v, w), pt in zip(regions, barys, points):
        use = region & ~taken
        bary = np.where(use[..., None], np.stack(np.broadcast_arrays(u, v, w), axis=-1), bary)
        point = np.where(use[..., None], pt, point)
        taken |= region
    d = p - point
    return _dot(d, d).astype(dt), point.astype(dt), bary.astype(dt)


def closest_point(vertices, faces, points, dtype=np.float64):
    """One frame: vertices (V, 3), faces (F, 3), points (Q, 3) -> dict of dist (Q,), face (Q,) -- the lowest d2, the lowest
    id on a tie --, bary (Q, 3), closest (Q, 3) and `all_dist` (Q, F), every face's own distance."""
    v = np.asarray(vertices, dtype=dtype)
    f = np.asarray(faces, dtype=np.int64)
    p = np.asarray(points, dtype=dtype)[:, None, :]
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    d2, point, bary = closest_pairs(p, a, b, c)
    face = np.argmin(d2, axis=1)                      # the first of equal values
    pick = np.arange(len(face))
    return {'dist': np.sqrt(d2[pick, face]), 'face': face, 'bary': bary[pick, face], 'closest': point[pick, face],
            'all_dist': np.sqrt(d2), 'all_closest': point}


# ---- inside ------------------------------------------------------------------------------------------------------------
def _edge(idf, f, idt, t, px, py):
    """The edge function of the directed edge f -> t at (px, py): formed from the endpoint with the lower vertex id, negated
    when the edge runs from the higher id to the lower."""
    swap = idf > idt
    lo = np.where(swap[..., None], t, f)
    hi = np.where(swap[..., None], f, t)
    e = (hi[..., 0] - lo[..., 0]) * (py - lo[..., 1]) - (hi[..., 1] - lo[..., 1]) * (px - lo[..., 0])
    return np.where(swap, -e, e)


def _owns(f, t):
    """Half-open rule: the oriented edge f -> t belongs to its face when it runs down in y, or level and towards +x."""
    return (t[..., 1] < f[..., 1]) | ((t[..., 1] == f[..., 1]) & (t[..., 0] > f[..., 0]))


def inside(vertices, faces, points):
    """Parity of the faces the ray from each point along +z crosses, float64 on the (float32) coordinates; (Q,) bool."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    f = np.asarray(faces, dtype=np.int64)
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    i0, i1, i2 = f[:, 0][None], f[:, 1][None], f[:, 2][None]
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    px, py, pz = p[:, 0][:, None], p[:, 1][:, None], p[:, 2][:, None]
    area = _edge(i0, a, i1, b, c[..., 0], c[..., 1])
    neg = area < 0
    sign = np.where(neg, -1.0, 1.0)
    w0 = sign * _edge(i0, a, i1, b, px, py)
    w1 = sign * _edge(i1, b, i2, c, px, py)
    w2 = sign * _edge(i2, c, i0, a, px, py)
    own0 = np.where(neg, _owns(b, a), _owns(a, b))
    own1 = np.where(neg, _owns(c, b), _owns(b, c))
    own2 = np.where(neg, _owns(a, c), _owns(c, a))
    covered = ((w0 > 0) | ((w0 == 0) & own0)) & ((w1 > 0) | ((w1 == 0) & own1)) & ((w2 > 0) | ((w2 == 0) & own2))
    above = (w0 * (c[..., 2] - pz) + w1 * (a[..., 2] - pz)) + w2 * (b[..., 2] - pz) > 0
    crossed = covered & above & (area != 0)
    return (crossed.sum(axis=1) % 2) == 1


# ---- meshes ------------------------------------------------------------------------------------------------------------
def tetrahedron():
    """Regular, centred on the origin, outward faces."""
    v = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float32) * 0.5
    f = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)
    return v, f


def cube():
    """The unit cube [0, 1]^3, 12 outward faces; the top face (z = 1) is split along the diagonal (0,0,1) - (1,1,1)."""
    v = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], dtype=np.float32)
    f = np.array([[0, 2, 3], [0, 3, 1],      # z = 0
                  [4, 5, 7], [4, 7, 6],      # z = 1
                  [0, 1, 5], [0, 5, 4],      # y = 0
                  [2, 6, 7], [2, 7, 3],      # y = 1
                  [0, 4, 6], [0, 6, 2],      # x = 0
                  [1, 3, 7], [1, 7, 5]], dtype=np.int32)
    return v, f


def octahedron():
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32) * 0.75
    f = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int32)
    return v, f


def icosahedron(subdivisions=1):
    """An icosahedron whose faces are split in four `subdivisions` times (80 faces for 1); the new vertices are NOT pushed
    out to the sphere, so the solid stays the convex icosahedron and the analytic half-space test holds."""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g],
         [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]]
    v = [np.asarray(x, dtype=np.float64) / np.sqrt(1.0 + g * g) for x in v]
    f = [[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
         [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
         [9, 8, 1]]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                v.append((v[i] + v[j]) / 2.0)
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
        f = out
    return np.asarray(v, dtype=np.float32), np.asarray(f, dtype=np.int32)


TORUS_R, TORUS_r = 1.0, 0.3


def torus(nu, nv):
    """Vertices on the analytic torus (axis z, R = 1, r = 0.3) on `torus_grid_faces(nu, nv)`: u goes round the tube."""
    u = (np.arange(nu) / nu * 2.0 * np.pi)[:, None]
    w = (np.arange(nv) / nv * 2.0 * np.pi)[None, :]
    ring = TORUS_R + TORUS_r * np.cos(u)
    xyz = np.stack([ring * np.cos(w), ring * np.sin(w), TORUS_r * np.sin(u) * np.ones_like(w)], axis=-1)
    return xyz.reshape(nu * nv, 3).astype(np.float32), torus_grid_faces(nu, nv).astype(np.int32)


def torus_faceting_error(nu, nv):
    """A bound on the distance between the analytic torus and its grid mesh: the sagitta of a chord round the tube plus that
    of a chord round the axis."""
    return TORUS_r * (1.0 - np.cos(np.pi / nu)) + (TORUS_R + TORUS_r) * (1.0 - np.cos(np.pi / nv))


def torus_signed_distance(points):
    p = np.asarray(points, dtype=np.float64)
    return np.hypot(np.hypot(p[:, 0], p[:, 1]) - TORUS_R, p[:, 2]) - TORUS_r


def torus_displaced(n, delta, seed):
    """n points on the analytic torus displaced by `delta` along the outward normal (negative: inwards), float32."""
    rng = np.random.default_rng(seed)
    u, w = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    normal = np.stack([np.cos(u) * np.cos(w), np.cos(u) * np.sin(w), np.sin(u)], axis=-1)
    centre = np.stack([TORUS_R * np.cos(w), TORUS_R * np.sin(w), np.zeros(n)], axis=-1)
    return (centre + (TORUS_r + delta) * normal).astype(np.float32)


def convex_planes(vertices, faces):
    """Outward unit normals n (F', 3) and offsets h of a convex polytope's faces: inside <=> n . p - h <= 0 for all."""
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    n = np.cross(b - a, c - a)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n *= np.sign(np.einsum('fk,fk->f', n, a - v.mean(axis=0)))[:, None]
    return n, np.einsum('fk,fk->f', n, a)


def convex_inside(vertices, faces, points):
    n, h = convex_planes(vertices, faces)
    return ((np.asarray(points, dtype=np.float64) @ n.T - h) <= 0).all(axis=1)


def convex_distance(vertices, faces, points, iterations=400):
    """The distance of each point to the SURFACE of a convex polytope without any triangle code.  Outside: the distance to
    the solid, by Dykstra's alternating projections onto its half-spaces (converges to the projection onto their
    intersection).  Inside: the smallest distance to a face plane."""
    n, h = convex_planes(vertices, faces)
    p = np.asarray(points, dtype=np.float64)
    out = np.empty(len(p))
    for k, x0 in enumerate(p):
        slack = n @ x0 - h
        if (slack <= 0).all():
            out[k] = -slack.max()
            continue
        x = x0.copy()
        corr = np.zeros((len(n), 3))
        for _ in range(iterations):
            for i in range(len(n)):
                y = x + corr[i]
                over = max(n[i] @ y - h[i], 0.0)
                x_new = y - over * n[i]
                corr[i] = y - x_new
                x = x_new
        out[k] = np.linalg.norm(x - x0)
    return out


def displaced_from_faces(vertices, faces, n, delta, seed):
    """n points at random barycentric positions strictly inside random faces, displaced by `delta` along the face's
    outward normal (convex meshes; negative: inwards), float32."""
    rng = np.random.default_rng(seed)
    v = np.asarray(vertices, dtype=np.float64)
    normals, _ = convex_planes(vertices, faces)
    pick = rng.integers(0, len(faces), n)
    w = rng.dirichlet([2.0, 2.0, 2.0], n)
    on = np.einsum('nk,nkd->nd', w, v[faces[pick]])
    return (on + delta * normals[pick]).astype(np.float32)


def grazing_rays():
    """Exactly representable rays on the unit cube that pass through vertices, along edges and vertical faces and through
    the diagonal of the top face, with the parity the half-open rule gives them: that of the ray displaced by (+eps,
    +eps^2), so a ray on the x = 0 or y = 0 side belongs to the cube and one on the x = 1 or y = 1 side does not."""
    rays = []
    for x in (0.0, 0.5, 1.0):
        for y in (0.0, 0.5, 1.0):
            column_inside = x < 1.0 and y < 1.0
            for z, between in ((-1.0, False), (0.5, True), (1.5, False)):
                rays.append(((x, y, z), column_inside and between))
    for x, y in ((0.25, 0.25), (0.75, 0.75), (0.25, 0.75)):                      # on and off the top face's diagonal
        rays += [((x, y, 0.25), True), ((x, y, -0.25), False), ((x, y, 1.25), False)]
    rays += [((-0.5, 0.5, 0.5), False), ((1.5, 1.0, 0.5), False), ((0.0, 1.5, 0.5), False)]
    points = np.array([r[0] for r in rays], dtype=np.float32)
    return points, np.array([r[1] for r in rays])


# ---- the queries of the GPU test ---------------------------------------------------------------------------------------
def special_queries(vertices, faces):
    """On a vertex, on an edge's midpoint, at a face's (0.25, 0.25, 0.5) point, the origin, and 100 m away."""
    v = np.asarray(vertices, dtype=np.float32)
    a, b, c = (v[faces[0, k]] for k in range(3))
    return np.stack([a, (a + b) * np.float32(0.5), np.float32(0.25) * a + np.float32(0.25) * b + np.float32(0.5) * c,
                     np.zeros(3, np.float32), np.array([60.0, -80.0, 100.0], np.float32)]).astype(np.float32)


def random_queries(n, seed, scale=1.5):
    return np.random.default_rng(seed).uniform(-scale, scale, size=(n, 3)).astype(np.float32)


def degenerate_mesh():
    """The cube plus a face without area (three collinear corners), a face with a repeated corner and a copy of face 0 at
    the end: no NaN may come out, and face 0 must beat its copy."""
    v, f = cube()
    v = np.concatenate([v, np.array([[0.5, 0.5, 2.0], [1.0, 1.0, 2.0], [1.5, 1.5, 2.0]], np.float32)])
    extra = np.array([[8, 9, 10], [8, 8, 9], f[0]], dtype=np.int32)
    return v, np.concatenate([f, extra]).astype(np.int32)


def gpu_cases():
    """[(name, vertices (T, V, 3), faces, points (T, Q, 3))]: the shapes of tests/test_surface_query.py.  F = 1, 4, 12, 80,
    510 and 516 (the workgroup's face stride is 512), 24 576 on 12 288 vertices (the largest frame a workgroup stages in LDS)
    and 24 642 on 12 321 vertices (the L2 path); Q = 1, 12, 13 (the query block is 12) and 64; T = 1 and 3 with different vertices per frame."""
    cases = []

    def frames(v, t, seed):
        rng = np.random.default_rng(seed)
        return np.stack([v] + [(v + rng.normal(0, 0.01, v.shape)).astype(np.float32) for _ in range(t - 1)])

    def queries(v, f, t, q, seed):
        rows = []
        for k in range(t):
            sp = special_queries(v[k], f)
            rows.append(np.concatenate([sp, random_queries(max(q - len(sp), 0), seed + k)])[:q])
        return np.stack(rows).astype(np.float32)
    tri = (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32), np.array([[0, 1, 2]], np.int32))
    for name, (v, f), t, q in (('triangle', tri, 1, 12), ('tetrahedron', tetrahedron(), 3, 1),
                               ('cube', cube(), 1, 13), ('icosahedron', icosahedron(1), 3, 64),
                               ('degenerate', degenerate_mesh(), 1, 12),
                               ('torus510', torus(15, 17), 1, 12), ('torus516', torus(6, 43), 3, 13),
                               ('torus_lds', torus(96, 128), 1, 12), ('torus_l2', torus(111, 111), 1, 12)):
        vt = frames(v, t, 5)
        cases.append((name, vt, f, queries(vt, f, t, q, 11)))
    # the regular tetrahedron's centroid, where its four faces tie
    v, f = tetrahedron()
    cases.append(('tetrahedron_centroid', v[None], f, np.zeros((1, 1, 3), np.float32)))
    cases.append(('body',) + synthetic_body())
    return cases


_BODY = []


def synthetic_body():
    """The synthetic stand-in body (V = 6890, F = 13 780) at rest in two shapes, and 12 readings per frame a centimetre or
    two off its vertices: (vertices (2, V, 3), faces, points (2, 12, 3)), built once."""
    if not _BODY:
        from em_pose_amd.synthetic import make_model
        model = make_model()
        rng = np.random.default_rng(21)
        betas = rng.normal(0.0, 1.0, size=(2, model['shapedirs'].shape[2]))
        v = model['v_template'][None].astype(np.float64) + np.einsum('vkb,tb->tvk', model['shapedirs'], betas)
        sites = rng.choice(v.shape[1], size=12, replace=False)
        points = v[:, sites] + rng.normal(0.0, 0.015, size=(2, 12, 3))
        _BODY.append((v.astype(np.float32), model['f'].astype(np.int32), points.astype(np.float32)))
    return _BODY[0]
