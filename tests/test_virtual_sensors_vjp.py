"""
VirtualMarkerHelper and vertex normals under autograd: the vector-Jacobian product of the virtual sensors
(empose_virtual_sensors_vjp, csrc/sensors_vjp.hip) against float64 autograd through the oracle
(oracle/torch_ref.py virtual_pos_and_rot, vertex_normals_sub, smpl_fk).

The bar, per frame row of d_vertices (or of g_poses and g_betas): the largest error of the row is at most 1e-4 x the
row's largest |g64|, and at most 4 x the error of float32 CPU autograd through the same oracle (the control) plus
1e-7 x the row's scale.
"""
import numpy as np
import pytest
import torch

from em_pose_amd import _lib, synthetic
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.data.virtual_sensors import VirtualMarkerHelper
from em_pose_amd.helpers.configuration import CONSTANTS as CONST
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


class _Stub(object):
    """What VirtualMarkerHelper reads of a body model: the faces."""

    def __init__(self, faces):
        self.model = {'f': np.asarray(faces, dtype=np.int64)}


@pytest.fixture(scope='module')
def model():
    return synthetic.make_model()


def _posed(model, n, seed, noise=0.003):
    """Posed synthetic meshes (float32 CPU oracle) plus per-vertex noise, (n, V, 3) float32."""
    rng = np.random.default_rng(seed)
    bm = R.BodyModelTensors(model, dtype=torch.float32)
    t = lambda a: torch.from_numpy(a.astype(np.float32))
    with torch.no_grad():
        v, _ = R.smpl_fk(bm, t(rng.normal(0, 0.3, (n, 63))), t(rng.normal(0, 1, (n, 10))), t(rng.normal(0, 0.5, (n, 3))))
    return (v.numpy() + rng.normal(0, noise, v.shape)).astype(np.float32)


def _cotangents(rng, n, m, which=('pos', 'ori', 'nor')):
    shapes = {'pos': (n, m, 3), 'ori': (n, m, 3, 3), 'nor': (n, m, 3)}
    return {k: (rng.normal(0, 1, shapes[k]).astype(np.float32) if k in which else None) for k in shapes}


def _oracle_dv(faces, verts, ids, cots, dtype):
    """d_vertices (n, V, 3) float64 of autograd through the oracle's virtual_pos_and_rot."""
    tables = R.sensor_tables(faces, ids)
    v = torch.from_numpy(verts.astype(np.float64)).to(dtype).requires_grad_(True)
    outs = R.virtual_pos_and_rot(v, ids, tables)
    loss = 0
    for out, key in zip(outs, ('pos', 'ori', 'nor')):
        if cots[key] is not None:
            loss = loss + (out * torch.from_numpy(cots[key]).to(dtype)).sum()
    loss.backward()
    return v.grad.numpy().astype(np.float64)


def _ours_dv(helper, verts, ids, cots):
    v = torch.from_numpy(verts).to(DEV).requires_grad_(True)
    outs = helper.get_virtual_pos_and_rot(v, ids)
    pairs = [(o, torch.from_numpy(cots[k]).to(DEV)) for o, k in zip(outs, ('pos', 'ori', 'nor')) if cots[k] is not None]
    torch.autograd.backward([p[0] for p in pairs], [p[1] for p in pairs])
    return v.grad.cpu().numpy().astype(np.float64)


def _check_rows(name, got, g64, g32):
    got, g64, g32 = (a.reshape(a.shape[0], -1) for a in (got, g64, g32))
    scale = np.abs(g64).max(axis=1)
    err = np.abs(got - g64).max(axis=1)
    err32 = np.abs(g32 - g64).max(axis=1)
    bad = np.nonzero((err > 1e-4 * scale) | (err > 4 * err32 + 1e-7 * scale))[0]
    assert bad.size == 0, '{}: rows {} err {} scale {} control {}'.format(
        name, bad[:8], err[bad[:8]], scale[bad[:8]], err32[bad[:8]])


def _check_helper(faces, helper, verts, ids, cots, name):
    got = _ours_dv(helper, verts, ids, cots)
    g64 = _oracle_dv(faces, verts, ids, cots, torch.float64)
    g32 = _oracle_dv(faces, verts, ids, cots, torch.float32)
    _check_rows(name, got, g64, g32)
    return got


def test_helper_model_sensors_all_and_each_cotangent(model):
    verts = _posed(model, 9, seed=1)
    helper = VirtualMarkerHelper(_Stub(model['f']))
    ids = list(CONST.VERTEX_IDS)
    rng = np.random.default_rng(2)
    for which in (('pos', 'ori', 'nor'), ('pos',), ('ori',), ('nor',)):
        cots = _cotangents(rng, verts.shape[0], len(ids), which)
        got = _check_helper(model['f'], helper, verts, ids, cots, '+'.join(which))
        untouched = np.ones(verts.shape[1], bool)
        sub_faces = R.sensor_tables(model['f'], ids)[0]
        untouched[sub_faces.reshape(-1)] = False
        assert not got[:, untouched].any()


def test_helper_shared_and_repeated_vertices(model):
    verts = _posed(model, 7, seed=3)
    helper = VirtualMarkerHelper(_Stub(model['f']))
    first = CONST.VERTEX_IDS[0]
    hv = helper.get_vertex_helpers([first])[0]
    # neighbours along the grid (overlapping faces), a sensor on another sensor's helper, a repeated id
    ids = [first, first + 1, first + 106, hv, 3748, first]
    assert len(set(ids)) < len(ids)
    cots = _cotangents(np.random.default_rng(4), verts.shape[0], len(ids))
    _check_helper(model['f'], helper, verts, ids, cots, 'shared')


def _irregular_mesh(rng):
    """A closed fan of 13 triangles (center of degree 13, rim vertices of degree 2), a triangle split at an inner point
    (degree 3), an open fan of 4 triangles (a boundary vertex of degree 4), gently curved so that no normal vanishes."""
    ring = 13
    pts = [[0, 0, 0.1]] + [[np.cos(2 * np.pi * i / ring), np.sin(2 * np.pi * i / ring), 0.05 * np.sin(3 * i)]
                           for i in range(ring)]
    faces = [[0, 1 + i, 1 + (i + 1) % ring] for i in range(ring)]
    o = len(pts)
    pts += [[3, 0, 0], [4, 0, 0.1], [3.5, 1, 0], [3.5, 0.3, 0.2]]
    faces += [[o, o + 1, o + 3], [o + 1, o + 2, o + 3], [o + 2, o, o + 3]]
    o = len(pts)
    pts += [[6, 0, 0.05]] + [[6 + np.cos(a), np.sin(a), 0.1 * a] for a in np.linspace(0, 2.5, 5)]
    faces += [[o, o + 1 + i, o + 2 + i] for i in range(4)]
    return np.asarray(pts), np.asarray(faces, dtype=np.int64)


def test_helper_irregular_mesh():
    rng = np.random.default_rng(5)
    pts, faces = _irregular_mesh(rng)
    counts = np.bincount(faces.reshape(-1))
    assert counts[0] == 13 and counts[17] == 3 and counts[18] == 4
    helper = VirtualMarkerHelper(_Stub(faces))
    ids = [0, 17, 18, 1, 14, 15, 18, 20, 22]
    verts = (pts[None] + rng.normal(0, 0.01, (5,) + pts.shape)).astype(np.float32)
    for which in (('pos', 'ori', 'nor'), ('ori',)):
        cots = _cotangents(rng, verts.shape[0], len(ids), which)
        _check_helper(faces, helper, verts, ids, cots, 'irregular ' + '+'.join(which))


def test_full_mesh_vertex_normals(model):
    smpl = SMPLLayer(model).to(DEV)
    verts = _posed(model, 5, seed=6)
    V = verts.shape[1]
    rng = np.random.default_rng(7)
    for ids in (None, [int(i) for i in rng.choice(V, 300, replace=False)]):
        m = V if ids is None else len(ids)
        d_nor = rng.normal(0, 1, (verts.shape[0], m, 3)).astype(np.float32)
        v = torch.from_numpy(verts).to(DEV).requires_grad_(True)
        nor = smpl.vertex_normals(v, ids)
        assert nor.grad_fn is not None
        nor.backward(torch.from_numpy(d_nor).to(DEV))
        got = v.grad.cpu().numpy().astype(np.float64)
        full = list(range(V)) if ids is None else ids
        cots = {'pos': None, 'ori': None, 'nor': d_nor}
        g64 = _oracle_dv(model['f'], verts, full, cots, torch.float64)
        g32 = _oracle_dv(model['f'], verts, full, cots, torch.float32)
        _check_rows('normals M={}'.format(m), got, g64, g32)


def _apply_offsets(pos, ori, o_r, o_t):
    """As get_estimated_real_markers (reference models.py:471-483)."""
    return pos + torch.matmul(ori, o_t[..., None])[..., 0], torch.matmul(ori, o_r)


def _well_conditioned_frames(model, ids, rng, n):
    """n random (poses [n][66] root first, betas [n][10]) whose sensor frames are well conditioned: at every sensor the
    direction to the helper is at least ~11 degrees away from the normal (|nh x s| >= 0.2).  Near that degeneracy the
    gradient amplifies the forward's own rounding of the vertices (about 1e-7) by 1/|nh x s|^2: at |nh x s| = 0.02 the
    float32 CPU control itself is off by 1e-3 in a row of scale 50, and which fp32 forward happens to round better
    decides the comparison, not the reverse under test."""
    bm = R.BodyModelTensors(model, dtype=torch.float64)
    tables = R.sensor_tables(model['f'], ids)
    keep_p, keep_b = [], []
    while len(keep_p) < n:
        pose = rng.normal(0, 0.3, (4 * n, 66)).astype(np.float32)
        betas = rng.normal(0, 1, (4 * n, 10)).astype(np.float32)
        t = lambda a: torch.from_numpy(a).double()
        with torch.no_grad():
            v, _ = R.smpl_fk(bm, t(pose[:, 3:]), t(betas), t(pose[:, :3]))
            nor = R.vertex_normals_sub(v, torch.from_numpy(tables[0]), torch.from_numpy(tables[1]))
            nh = nor / nor.norm(dim=-1, keepdim=True)
            sd = v[:, tables[2].tolist()] - v[:, ids]
            sd = sd / sd.norm(dim=-1, keepdim=True)
            ok = (torch.cross(nh, sd, dim=-1).norm(dim=-1).min(dim=1).values >= 0.2).numpy()
        keep_p += list(pose[ok]); keep_b += list(betas[ok])
    return np.stack(keep_p[:n]), np.stack(keep_b[:n])


def test_end_to_end_smpl_helper_offsets(model):
    from em_pose_amd.helpers.configuration import lgd_config
    from em_pose_amd.nn.models import _SmplSensorsFn, create_model
    n, ids = 11, list(CONST.VERTEX_IDS)
    rng = np.random.default_rng(8)
    pose, betas = _well_conditioned_frames(model, ids, rng, n)
    q, _ = np.linalg.qr(rng.normal(size=(12, 3, 3)))
    o_r = q.astype(np.float32)[None]
    o_t = rng.normal(0, 0.02, (1, 12, 3)).astype(np.float32)
    d_pos = rng.normal(0, 1, (n, 12, 3)).astype(np.float32)
    d_ori = rng.normal(0, 1, (n, 12, 3, 3)).astype(np.float32)

    def oracle(dtype, at=None):
        """autograd through the oracle; with `at` the sensors are evaluated at those vertices (the SMPL Jacobian stays
        the oracle's own): what the reverse computes from the vertices our forward produced."""
        bm = R.BodyModelTensors(model, dtype=dtype)
        p = torch.from_numpy(pose).to(dtype).requires_grad_(True)
        b = torch.from_numpy(betas).to(dtype).requires_grad_(True)
        c = lambda a: torch.from_numpy(a).to(dtype)
        v, _ = R.smpl_fk(bm, p[:, 3:], b, p[:, :3])
        if at is not None:
            v = v + (c(at) - v.detach())
        pos, ori, _ = R.virtual_pos_and_rot(v, ids, R.sensor_tables(model['f'], ids))
        pos_c, ori_c = _apply_offsets(pos, ori, c(o_r), c(o_t))
        ((pos_c * c(d_pos)).sum() + (ori_c * c(d_ori)).sum()).backward()
        return p.grad.numpy().astype(np.float64), b.grad.numpy().astype(np.float64)

    smpl = SMPLLayer(model).to(DEV)
    helper = VirtualMarkerHelper(smpl)
    p = torch.from_numpy(pose).to(DEV).requires_grad_(True)
    b = torch.from_numpy(betas).to(DEV).requires_grad_(True)
    v, _ = smpl(poses_body=p[:, 3:], betas=b, poses_root=p[:, :3])
    pos, ori, _ = helper.get_virtual_pos_and_rot(v, ids)
    pos_c, ori_c = _apply_offsets(pos, ori, torch.from_numpy(o_r).to(DEV), torch.from_numpy(o_t).to(DEV))
    ((pos_c * torch.from_numpy(d_pos).to(DEV)).sum() + (ori_c * torch.from_numpy(d_ori).to(DEV)).sum()).backward()
    ours = p.grad.cpu().numpy().astype(np.float64), b.grad.cpu().numpy().astype(np.float64)
    g64 = oracle(torch.float64)
    for name, a, w in zip(('g_poses', 'g_betas'), ours, g64):
        scale = np.abs(w).max(axis=1)
        assert (np.abs(a - w).max(axis=1) <= 1e-4 * scale).all(), name
    # The full bar once the forward's own rounding is taken out of the comparison: float64 and float32 autograd through
    # the oracle with the sensors at the vertices our forward produced.  (Against the plain float64 gradient the fp32
    # rounding of the vertices, about 1e-7, differs between our forward and the CPU's and dominates the comparison.)
    at = v.detach().cpu().numpy()
    for name, a, w, c in zip(('g_poses', 'g_betas'), ours, oracle(torch.float64, at), oracle(torch.float32, at)):
        _check_rows(name + ' at our vertices', a, w, c)

    # the LGD model's own analytic reverse over the sensor sub-mesh, on the same body model
    net = create_model(lgd_config(12, False, 1, hidden=32), smpl).to(DEV).eval()
    net.vertex_ids = ids
    p2 = torch.from_numpy(pose).to(DEV).requires_grad_(True)
    b2 = torch.from_numpy(betas).to(DEV).requires_grad_(True)
    pos2, ori2, _ = _SmplSensorsFn.apply(net, p2, b2, torch.from_numpy(o_r).to(DEV), torch.from_numpy(o_t).to(DEV), n)
    ((pos2 * torch.from_numpy(d_pos).to(DEV)).sum() + (ori2 * torch.from_numpy(d_ori).to(DEV)).sum()).backward()
    lgd = p2.grad.cpu().numpy().astype(np.float64), b2.grad.cpu().numpy().astype(np.float64)
    for name, a, c, w in zip(('g_poses', 'g_betas'), ours, lgd, g64):
        scale = np.abs(w).max(axis=1)
        e_lgd, e_ab = np.abs(c - w).max(axis=1), np.abs(a - c).max(axis=1)
        assert (e_lgd <= 1e-4 * scale).all(), 'LGD path {}: {}'.format(name, e_lgd / scale)
        assert (e_ab <= 2e-4 * scale).all(), 'helper path vs LGD path {}: {}'.format(name, e_ab / scale)


def test_determinism_and_no_interference(model):
    smpl = SMPLLayer(model).to(DEV)
    helper = VirtualMarkerHelper(smpl)
    ids = list(CONST.VERTEX_IDS)
    verts = torch.from_numpy(_posed(model, 13, seed=9)).to(DEV)   # odd T
    rng = np.random.default_rng(10)
    cots = [torch.from_numpy(c).to(DEV) for c in _cotangents(rng, 13, 12).values()]

    def grad(v):
        x = v.clone().requires_grad_(True)
        torch.autograd.backward(list(helper.get_virtual_pos_and_rot(x, ids)), cots)
        return x.grad

    a, b = grad(verts), grad(verts)
    assert torch.equal(a, b)
    V = verts.shape[1]
    d_nor = torch.from_numpy(rng.normal(0, 1, (13, V, 3)).astype(np.float32)).to(DEV)
    x1, x2 = verts.clone().requires_grad_(True), verts.clone().requires_grad_(True)
    smpl.vertex_normals(x1).backward(d_nor)
    smpl.vertex_normals(x2).backward(d_nor)
    assert torch.equal(x1.grad, x2.grad)

    # with grad the outputs are those of a no-grad call, bit for bit; without an input that requires grad, no node
    with torch.no_grad():
        plain = helper.get_virtual_pos_and_rot(verts, ids)
    x = verts.clone().requires_grad_(True)
    tracked = helper.get_virtual_pos_and_rot(x, ids)
    for p_, t_ in zip(plain, tracked):
        assert t_.grad_fn is not None and torch.equal(p_, t_.detach())
    for o in helper.get_virtual_pos_and_rot(verts, ids):
        assert o.grad_fn is None and not o.requires_grad
    assert smpl.vertex_normals(verts).grad_fn is None

    # float64 vertices: the gradient comes back in the caller's dtype and shape
    x = verts.double().requires_grad_(True)
    helper.get_virtual_pos_and_rot(x, ids)[0].backward(cots[0])
    assert x.grad.dtype == torch.float64 and x.grad.shape == x.shape
    x32 = verts.clone().requires_grad_(True)
    helper.get_virtual_pos_and_rot(x32, ids)[0].backward(cots[0])
    assert torch.equal(x.grad.float(), x32.grad)

    # CPU tensors are refused
    with pytest.raises(_lib.EmposeError):
        helper.get_virtual_pos_and_rot(verts.cpu().requires_grad_(True), ids)


def _vjp_rows(helper, verts, ids, cots):
    x = verts.clone().requires_grad_(True)
    outs = helper.get_virtual_pos_and_rot(x, ids)
    torch.autograd.backward([o for o, c in zip(outs, cots) if c is not None], [c for c in cots if c is not None])
    return x.grad


def test_frames_above_one_slab(model):
    """Full-mesh normals (M = V: 541 frames per slab) and 12 sensors (16384 frames per slab): every frame's rows are
    those of the same frames evaluated alone, and sampled frames match float64."""
    smpl = SMPLLayer(model).to(DEV)
    V = model['v_template'].shape[0]
    base = torch.from_numpy(_posed(model, 4, seed=11)).to(DEV)
    rng = np.random.default_rng(12)
    for ids, T in ((list(range(V)), 1101), (list(CONST.VERTEX_IDS), 16389)):
        helper = VirtualMarkerHelper(smpl)
        verts = base.repeat((T + 3) // 4, 1, 1)[:T].contiguous()
        verts = verts + 1e-3 * torch.randn(verts.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(T))
        d_nor = torch.randn(T, len(ids), 3, device=DEV, generator=torch.Generator(DEV).manual_seed(1))
        d_pos = torch.randn(T, len(ids), 3, device=DEV, generator=torch.Generator(DEV).manual_seed(2))
        cots = (d_pos, None, d_nor)
        whole = _vjp_rows(helper, verts, ids, cots)
        cut = T // 2 + 1
        for lo, hi in ((0, cut), (cut, T)):
            part = _vjp_rows(helper, verts[lo:hi], ids, tuple(c[lo:hi] if c is not None else None for c in cots))
            assert torch.equal(whole[lo:hi], part), (len(ids), lo, hi)
        frames = [0, cut, T - 1]
        sample = verts[frames].cpu().numpy()
        c = {'pos': d_pos[frames].cpu().numpy(), 'ori': None, 'nor': d_nor[frames].cpu().numpy()}
        g64 = _oracle_dv(model['f'], sample, ids, c, torch.float64)
        g32 = _oracle_dv(model['f'], sample, ids, c, torch.float32)
        _check_rows('slabs M={}'.format(len(ids)), whole[frames].cpu().numpy().astype(np.float64), g64, g32)
        del whole, verts
