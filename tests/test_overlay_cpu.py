"""CPU-side checks of the overlay ray caster: the conditions on the float64 restatement (tests/overlay_ref.py) and on its
scenes that tests/test_overlay.py rests on, the refusals of the C entry point, the descriptor's layout and the builders
of em_pose_amd/vis/overlay.py.  Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from em_pose_amd import _lib, synthetic
from em_pose_amd.bodymodels import tables as TB
from em_pose_amd.vis import overlay as OV
from oracle import torch_ref as R
from tests import overlay_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPOSE_EINVAL = -1   # include/empose_hip.h
EYE3, ZERO3 = np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32)


def _scene_primitives(scene):
    model = synthetic.make_model(nu=OR.NU, nv=OR.NV)
    bm = R.BodyModelTensors(model, dtype=torch.float64)
    root, body, betas = (torch.from_numpy(a).double() for a in OR.scene_inputs(scene))
    joints = R.smpl_fk(bm, body, betas, root)[1].numpy()
    return OR.scene_primitives(scene, joints, TB.model_parents(model))


# ---- the conditions of the GPU scenes -------------------------------------------------------------------------------
@pytest.mark.parametrize('scene', OR.SCENES, ids=[s.name for s in OR.SCENES])
def test_scene_conditions(scene):
    """What tests/test_overlay.py assumes, on the oracle's float64 body model.  Per frame: the ambiguity mask holds at
    most 3 % of the pixels covered or masked; outside it the float32 control picks the float64 primitive at every pixel,
    background included, and its depth is within 2e-5 relative (a cap: a badly conditioned formula must not pass by
    spoiling control and kernel alike); every float64 hit point lies on its capsule within 1e-9; and along a random
    sample of rays no point in front of the hit lies inside any primitive.

    Measured (covered pixels, mask share, control's largest relative depth error; frames in order):
      one_frame 75, 1.3 %, 1.1e-7;  three_frames 269 / 313 / 309, 0.7 / 0.6 / 1.9 %, 1.2e-7;  close_up 4237, 1.8 %, 3.3e-7;
      wide_angle 344, 0.6 %, 1.4e-6;  leaves_image 62, 1.6 %, 3.3e-7;  camera_per_frame 63 / 65 / 75, 1.6 / 0 / 0 %, 1.2e-7;
      partial_tiles 246, 0.8 %, 2.1e-7.
    The same control with the quadratics formed about the eye (shift=False) is 7e-5 to 4e-4 off in depth on these scenes
    and picks another primitive at clear pixels of five of the eleven frames: the origin shift is what the kernel needs."""
    prims = _scene_primitives(scene)
    assert 150 <= prims.n_primitives <= 250
    f64 = OR.reference_frames(scene, prims)
    f32 = OR.reference_frames(scene, prims, dtype=np.float32, ambiguity=False)
    cam = OR.scene_camera(scene)
    rng = np.random.default_rng(scene.seed + 900)
    a_w, b_w, radii = prims.a.numpy(), prims.b.numpy(), prims.radius.numpy().astype(np.float64)
    for k, (ref, ctl) in enumerate(zip(f64, f32)):
        Rk, tk = (cam.R[k], cam.t[k]) if cam.R.ndim == 3 else (cam.R, cam.t)
        radius = radii[k] if radii.ndim == 2 else radii
        share = ref.ambiguous.sum() / float((ref.covered | ref.ambiguous).sum())
        clear = ~ref.ambiguous
        same = clear & ref.covered & (ctl.prim_id == ref.prim_id)
        err = float(np.max(np.abs(ctl.prim_depth[same].astype(np.float64) - ref.prim_depth[same]) / ref.prim_depth[same]))
        print('{} frame {}: P {}, covered {}, masked {} ({:.2f} %), control depth error {:.2e}'
              .format(scene.name, k, prims.n_primitives, ref.covered.sum(), ref.ambiguous.sum(), 100 * share, err))
        assert ref.covered.sum() >= 50 and len(np.unique(ref.prim_id)) >= 30
        assert share <= OR.MASK_CAP
        assert np.array_equal(ctl.prim_id[clear], ref.prim_id[clear])
        assert err <= 2e-5
        assert not ref.near_band.any()
        # every hit point s d lies on its capsule
        a_c, b_c = OR.camera_space(a_w[k], Rk, tk, np.float64), OR.camera_space(b_w[k], Rk, tk, np.float64)
        dx, dy, _ = OR.rays(cam.fx, cam.fy, cam.cx, cam.cy, scene.H, scene.W, np.float64)
        d = np.stack([np.broadcast_to(dx, ref.covered.shape), np.broadcast_to(dy, ref.covered.shape),
                      np.ones(ref.covered.shape)], axis=-1)
        ii, jj = np.nonzero(ref.covered)
        ids = ref.prim_id[ii, jj]
        points = ref.prim_depth[ii, jj][:, None] * d[ii, jj]
        off = OR.distance_to_segment(points, a_c[ids], b_c[ids]) - radius[ids]
        assert np.abs(off).max() <= 1e-9
        # nothing in front of the hit: 48 points on each sampled ray between the near plane and the hit (or 8 m)
        pick = rng.choice(scene.H * scene.W, size=150, replace=False)
        if len(ii) > 150:
            hit_pick = rng.choice(len(ii), size=150, replace=False)
            pick = np.concatenate([pick, ii[hit_pick] * scene.W + jj[hit_pick]])
        pi, pj = pick // scene.W, pick % scene.W
        end = np.where(ref.covered[pi, pj], ref.prim_depth[pi, pj], 8.0)
        frac = (np.arange(48) + 0.5) / 48.0
        s = cam.near + (end[:, None] * (1 - 1e-9) - cam.near) * frac[None, :]
        pts = (s[..., None] * d[pi, pj][:, None, :]).reshape(-1, 3)
        drawn = radius > 0
        dist = OR.distance_to_segment(pts[:, None, :], a_c[drawn][None], b_c[drawn][None])
        assert (dist - radius[drawn][None] >= -1e-9).all()
    proj = lambda p_c: (cam.fx * p_c[:, 0] / p_c[:, 2] + cam.cx, cam.fy * p_c[:, 1] / p_c[:, 2] + cam.cy)
    last = f64[-1]
    if scene.name == 'close_up':        # tens of pixels wide, over several tiles
        widest = max((last.prim_id == p).any(axis=0).sum() for p in np.unique(last.prim_id) if p >= 0)
        assert widest >= 20
    if scene.name == 'wide_angle':
        assert cam.fx == scene.W / 4.0
        for corner in (last.covered[:8, :8], last.covered[:8, -8:], last.covered[-8:, :8], last.covered[-8:, -8:]):
            assert corner.any()
    if scene.name == 'leaves_image':
        assert (proj(a_c)[0] > scene.W).sum() >= 5 and last.covered[:, -1].any()
    if scene.name == 'partial_tiles':
        assert scene.H % 16 and scene.W % 16 and last.covered[48:].any() and last.covered[:, 64:].any()


def _one(a, b, r, H_=9, W_=9, near=0.05, f=8.0, c=4.5, dtype=np.float64, **kw):
    """Identity camera, fx = fy = f, cx = cy = c: with f = 8 and c = 4.5 the centre of pixel (4, 4) is the optical axis."""
    n = len(r)
    return OR.overlay_frame(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(r, np.float32),
                            np.tile(np.array([[0.5, 0.25, 1.0]], np.float32), (n, 1)), EYE3, ZERO3, f, f, c, c, near,
                            H_, W_, dtype=dtype, **kw)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_the_reference_on_hand_computed_cases(dtype):
    fr = _one([[0, 0, 2]], [[0, 0, 2]], [0.5], dtype=dtype)
    assert fr.prim_depth[4, 4] == 1.5 and fr.prim_id[4, 4] == 0      # the sphere's pole on the optical axis
    assert np.all(fr.rgb[4, 4] == [128, 64, 255])                     # n = -z = the light: the base colour itself
    assert fr.covered.sum() < 81 and np.all(fr.rgb[~fr.covered] == 255) and np.all(np.isinf(fr.prim_depth[~fr.covered]))
    # a pixel whose ray passes the centre at the distance rho sees the sphere iff rho <= r
    dx, dy, dd = OR.rays(8.0, 8.0, 4.5, 4.5, 9, 9, np.float64)
    rho2 = 4.0 - 4.0 / dd                                             # |c|^2 - (c . d)^2 / d.d with c = (0, 0, 2)
    assert np.array_equal(fr.covered, rho2 <= 0.25)
    # 40 identical spheres: the lowest index; a skipped first primitive: the next
    fr = _one([[0, 0, 2]] * 40, [[0, 0, 2]] * 40, [0.5] * 40, dtype=dtype)
    assert np.all(fr.prim_id[fr.covered] == 0) and np.all(fr.ambiguous[fr.covered])
    for bad in (0.0, -0.5, float('nan'), float('inf')):
        fr = _one([[0, 0, 2]] * 2, [[0, 0, 2]] * 2, [bad, 0.5], dtype=dtype)
        assert np.all(fr.prim_id[fr.covered] == 1) and fr.covered.any()
    fr = _one([[float('nan'), 0, 2]], [[0, 0, 2]], [0.5], dtype=dtype)
    assert not fr.covered.any()
    # about the camera, and behind it: nothing
    assert not _one([[0, 0, 0]], [[0, 0, 0]], [0.5], dtype=dtype).covered.any()
    assert not _one([[0, 0, -2]], [[0, 0, -2]], [0.5], dtype=dtype).covered.any()
    # along the optical axis: the side quadratic has the leading coefficient 0 on the axis, the cap is hit
    fr = _one([[0, 0, 2]], [[0, 0, 3]], [0.5], dtype=dtype)
    assert fr.prim_depth[4, 4] == 1.5
    # a capsule through the near plane: only where the entry is beyond it
    fr = _one([[-1, 0, 0.25]], [[1, 0, 1.25]], [0.125], near=0.75, dtype=dtype)
    assert fr.covered.any() and np.all(fr.prim_depth[fr.covered] > 0.75)
    assert fr.covered[4, 7:].all() and not fr.covered[4, :3].any()


def test_occlusion_in_the_reference():
    rgb_in = np.full((9, 9, 3), 40, np.uint8)
    two = dict(a=[[0, 0, 2], [0.5, 0, 2.5]], b=[[0, 0, 2], [0.5, 0, 2.5]], r=[0.5, 0.5])
    plain = _one(two['a'], two['b'], two['r'], rgb_in=rgb_in)
    assert plain.prim_depth[4, 4] == 1.5
    depth2 = np.full((9, 9), 2.0, np.float32)
    hidden = _one(two['a'], two['b'], two['r'], rgb_in=rgb_in, mesh_depth=depth2, hidden_alpha=0.0)
    front = plain.covered & (plain.prim_depth < 2.0)
    assert front.any() and (plain.covered & ~front).any()
    assert np.array_equal(hidden.rgb[front], plain.rgb[front]) and np.all(hidden.rgb[~front] == 40)
    xray = _one(two['a'], two['b'], two['r'], rgb_in=rgb_in, mesh_depth=depth2, hidden_alpha=1.0)
    assert np.array_equal(xray.rgb, plain.rgb)
    half = _one(two['a'], two['b'], two['r'], rgb_in=rgb_in, mesh_depth=depth2, hidden_alpha=0.5)
    back = plain.covered & ~front
    want = np.floor(0.5 * 40 + 0.5 * (plain.rgb[back].astype(float)) + 0.5)
    assert np.abs(half.rgb[back].astype(float) - want).max() <= 1          # (plain.rgb is itself rounded)
    inf = _one(two['a'], two['b'], two['r'], rgb_in=rgb_in, mesh_depth=np.full((9, 9), np.inf, np.float32))
    assert np.array_equal(inf.rgb, plain.rgb)
    # a hit at exactly the mesh depth is hidden: the tie goes to the mesh
    tie = _one([[0, 0, 2.5]], [[0, 0, 2.5]], [0.5], rgb_in=rgb_in, mesh_depth=depth2)
    assert tie.prim_depth[4, 4] == 2.0 and np.all(tie.rgb[4, 4] == 40)


# ---- the C entry point without a GPU --------------------------------------------------------------------------------
def _desc(keep, **change):
    """A descriptor every check accepts; the pointers are host memory that a refused call never reads."""
    buf = np.zeros(4096, np.float32)
    keep.append(buf)
    p = ctypes.c_void_p(buf.ctypes.data)
    d = _lib.OverlayDesc()
    d.T, d.P, d.H, d.W = 2, 5, 8, 12
    d.seg_a, d.seg_b, d.radius, d.radius_per_frame, d.colors = p, p, p, 0, p
    d.cam_R, d.cam_t, d.camera_per_frame = p, p, 0
    d.fx, d.fy, d.cx, d.cy, d.near = 10.0, 10.0, 6.0, 4.0, 0.05
    d.light[:], d.ambient, d.hidden_alpha = (0.0, 0.0, -1.0), 0.3, 0.5
    d.mesh_depth, d.slab_frames = p, 0
    d.rgb, d.prim_id, d.prim_depth = p, p, p
    for k, v in change.items():
        if k == 'light':
            d.light[:] = v
        else:
            setattr(d, k, v)
    return d, p


_up = lambda n: -(-n // 256) * 256      # the workspace is carved in pieces of 256 bytes


def test_bad_overlay_descriptors_are_refused_without_a_gpu():
    lib = _lib.lib()
    keep = []
    nbytes = lib.empose_render_overlay_workspace_bytes(2, 5, 8, 12)
    assert nbytes == _up(2 * 5 * 8 * 4) + _up(2 * 5 * 4 * 4)        # camera-space primitives and boxes of one slab

    def call(ws_size=None, ws=True, **change):
        d, p = _desc(keep, **change)
        return lib.empose_render_overlay(ctypes.byref(d), p if ws else None,
                                         ctypes.c_size_t(nbytes if ws_size is None else ws_size), None)
    assert lib.empose_render_overlay(None, None, 0, None) == EMPOSE_EINVAL
    for name in ('seg_a', 'seg_b', 'radius', 'colors', 'cam_R', 'cam_t', 'rgb'):
        assert call(**{name: None}) == EMPOSE_EINVAL, name
        assert b'null' in lib.empose_last_error()
    for name in ('T', 'P', 'H', 'W'):
        for bad in (0, -3):
            assert call(**{name: bad}) == EMPOSE_EINVAL, name
    assert call(P=_lib.OVERLAY_MAX_PRIMS + 1) == EMPOSE_EINVAL and b'cap' in lib.empose_last_error()
    assert call(H=_lib.RENDER_MAX_IMAGE + 1) == EMPOSE_EINVAL and b'cap' in lib.empose_last_error()
    assert call(W=_lib.RENDER_MAX_IMAGE + 1) == EMPOSE_EINVAL
    for bad in (-0.1, 1.5, float('nan')):
        assert call(hidden_alpha=bad) == EMPOSE_EINVAL and b'hidden_alpha' in lib.empose_last_error()
    for bad in (0.0, float('nan'), float('inf')):
        assert call(fx=bad) == EMPOSE_EINVAL and call(fy=bad) == EMPOSE_EINVAL
    for bad in (0.0, -0.05, float('nan'), float('inf')):
        assert call(near=bad) == EMPOSE_EINVAL and b'near' in lib.empose_last_error()
    assert call(light=(0.0, 0.0, 0.0)) == EMPOSE_EINVAL and call(light=(float('nan'), 0.0, 1.0)) == EMPOSE_EINVAL
    assert call(ambient=1.5) == EMPOSE_EINVAL and call(slab_frames=-1) == EMPOSE_EINVAL
    assert call(ws=False) == EMPOSE_EINVAL
    assert call(ws_size=nbytes - 1) == EMPOSE_EINVAL and b'workspace' in lib.empose_last_error()


def test_overlay_workspace_query():
    lib = _lib.lib()
    for T, P, H_, W_ in ((0, 5, 8, 8), (2, 0, 8, 8), (2, 5, 0, 8), (2, 5, 8, -1), (-1, 5, 8, 8),
                         (2, _lib.OVERLAY_MAX_PRIMS + 1, 8, 8), (2, 5, _lib.RENDER_MAX_IMAGE + 1, 8),
                         (2, 5, 8, _lib.RENDER_MAX_IMAGE + 1)):
        assert lib.empose_render_overlay_workspace_bytes(T, P, H_, W_) == 0
    # slabs of frames: bounded whatever T is
    big = lib.empose_render_overlay_workspace_bytes(10 ** 6, _lib.OVERLAY_MAX_PRIMS, 512, 512)
    assert 0 < big <= (16 << 20) + 512
    assert big == lib.empose_render_overlay_workspace_bytes(10 ** 5, _lib.OVERLAY_MAX_PRIMS, 512, 512)


def test_overlay_desc_matches_the_header_field_order():
    text = open(os.path.join(ROOT, 'include', 'empose_hip.h')).read()
    end = re.search(r'\}\s*empose_overlay_desc;', text).start()
    body = text[text.rfind('typedef struct {', 0, end) + len('typedef struct {'):end]
    names = []
    for decl in re.sub(r'/\*.*?\*/', '', body, flags=re.S).split(';'):
        for part in decl.strip().split(','):
            if part.strip():
                names.append(re.findall(r'([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[[^\]]*\])*\s*$', part.strip())[0])
    assert names == [f[0] for f in _lib.OverlayDesc._fields_]
    assert int(re.search(r'#define EMPOSE_OVERLAY_MAX_PRIMS (\d+)', text).group(1)) == _lib.OVERLAY_MAX_PRIMS


# ---- the builders, plain torch ------------------------------------------------------------------------------------------
def test_builders_shapes_and_masking():
    rng = np.random.default_rng(5)
    T, J, M = 3, 7, 4
    joints = torch.from_numpy(rng.normal(size=(T, J, 3)).astype(np.float32))
    parents = [-1, 0, 1, 1, 3, 0, 5]
    sk = OV.skeleton_primitives(joints, parents, bone_radius=0.01, joint_radius=0.03)
    assert sk.n_frames == T and sk.n_primitives == 6 + 7 and tuple(sk.radius.shape) == (13,)
    assert torch.equal(sk.a[:, :6], joints[:, [0, 1, 1, 3, 0, 5]]) and torch.equal(sk.b[:, :6], joints[:, 1:])
    assert torch.equal(sk.a[:, 6:], joints) and torch.equal(sk.b[:, 6:], joints)          # a == b: spheres
    assert torch.allclose(sk.radius, torch.tensor([0.01] * 6 + [0.03] * 7)) and tuple(sk.colors.shape) == (13, 3)

    pos = torch.from_numpy(rng.normal(size=(T, M, 3)).astype(np.float32))
    ori = torch.from_numpy(OR._rotations(rng, (T, M)).astype(np.float32))
    mask = torch.ones(T, M)
    mask[1, 2] = 0
    pos[2, 0] = -7.0                                           # the value missing sensors read in this batch
    se = OV.sensor_primitives(pos, ori, mask=mask, axis_length=0.1, mask_value=-7.0)
    assert se.n_primitives == 4 * M and tuple(se.radius.shape) == (T, 4 * M)
    gone = torch.zeros(T, M, dtype=torch.bool)
    gone[1, 2] = gone[2, 0] = True
    for block, r in enumerate((0.015, 0.004, 0.004, 0.004)):
        got = se.radius[:, block * M:(block + 1) * M]
        assert torch.all(got[gone] == 0) and torch.allclose(got[~gone], torch.tensor(r))
    for k in range(3):          # axis k ends at pos + 0.1 * column k of the rotation, in red, green, blue
        assert torch.allclose(se.b[:, (k + 1) * M:(k + 2) * M], pos + 0.1 * ori[..., :, k], atol=1e-6)
        assert torch.equal(se.colors[(k + 1) * M:(k + 2) * M].argmax(dim=1), torch.full((M,), k))
    assert torch.equal(se.a[:, :M], pos) and torch.equal(se.b[:, :M], pos)
    assert torch.all(OV.sensor_primitives(pos, ori.reshape(T, M * 9)).radius > 0)      # flattened rotations, no mask

    pos_hat = pos + 0.05
    re_ = OV.residual_primitives(pos, pos_hat, mask=mask, radius=0.006, mask_value=-7.0)
    assert re_.n_primitives == M and torch.equal(re_.a, pos) and torch.equal(re_.b, pos_hat)
    assert torch.all(re_.radius[gone] == 0) and torch.allclose(re_.radius[~gone], torch.tensor(0.006))

    every = OV.Primitives.cat(sk, [se, None], re_)
    assert every.n_primitives == 13 + 4 * M + M and tuple(every.radius.shape) == (T, 13 + 5 * M)
    assert torch.equal(every.radius[:, :13], sk.radius.expand(T, 13)) and torch.equal(every.colors[13:13 + 4 * M], se.colors)
    part = every.frames(slice(1, 3))
    assert part.n_frames == 2 and torch.equal(part.a, every.a[1:3]) and torch.equal(part.radius, every.radius[1:3])
    assert tuple(OV.Primitives.cat(sk, sk).radius.shape) == (26,)
    with pytest.raises(ValueError):
        OV.Primitives(torch.zeros(2, 3, 3), torch.zeros(2, 4, 3), 0.1, (1, 1, 1))
    with pytest.raises(ValueError):
        OV.Primitives.cat(sk, OV.Primitives(torch.zeros(2, 1, 3), torch.zeros(2, 1, 3), 0.1, (1, 1, 1)))


def test_cpu_tensors_raise():
    prims = OV.Primitives(torch.zeros(1, 1, 3), torch.zeros(1, 1, 3), 0.1, (1.0, 0.0, 0.0))
    from em_pose_amd.vis.camera import pinhole
    with pytest.raises(_lib.EmposeError):
        OV.draw_primitives(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), prims, pinhole(8, 8))
