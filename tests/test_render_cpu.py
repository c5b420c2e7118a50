"""CPU-side checks of the mesh renderer: the float64 restatement itself (tests/raster_ref.py) on hand-computed cases, the
conditions the GPU scenes of tests/test_render.py rest on, the refusals of the C entry point, the camera helpers and
the image output.  Nothing here needs a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from em_pose_amd import _lib, synthetic
from em_pose_amd.vis import camera as CAM
from em_pose_amd.vis import io as VIO
from oracle import torch_ref as R
from tests import helpers as H
from tests import raster_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPOSE_EINVAL = -1   # include/empose_hip.h
EYE3, ZERO3 = np.eye(3, dtype=np.float32), np.zeros(3, dtype=np.float32)


def _frame(vertices, faces, H_, W_, near=0.05, dtype=np.float64, **kw):
    """Identity camera with fx = fy = 1, cx = cy = 0: a vertex at Z = 1 lands at (X, Y)."""
    return RR.raster_frame(np.asarray(vertices, np.float32), np.asarray(faces), EYE3, ZERO3, 1.0, 1.0, 0.0, 0.0, near,
                           H_, W_, dtype=dtype, **kw)


# ---- the reference itself -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_one_triangle_covers_the_hand_computed_pixels_edges_included(dtype):
    # corners (0, 0), (4, 0), (0, 4): the centre (j + 0.5, i + 0.5) is inside where i + j + 1 <= 4, and the centres with
    # i + j = 3 lie exactly ON the hypotenuse x + y = 4 -- inclusive edges keep them
    fr = _frame([[0, 0, 1], [4, 0, 1], [0, 4, 1]], [[0, 1, 2]], 5, 5, dtype=dtype, colors=(0.5, 0.25, 1.0))
    ii, jj = np.indices((5, 5))
    want = ii + jj <= 3
    assert want.sum() == 10
    assert np.array_equal(fr.face_id >= 0, want) and np.array_equal(fr.covered, want)
    assert np.all(fr.face_id[want] == 0) and np.all(fr.face_id[~want] == -1)
    assert np.all(fr.depth[want] == 1.0) and np.all(np.isinf(fr.depth[~want]))
    assert np.all(fr.ambiguous[ii + jj == 3])          # on the edge line: what float32 may decide otherwise
    assert not fr.ambiguous[1, 1] and not fr.ambiguous[4, 4]
    # the other winding covers the same pixels: the edge functions are oriented by the sign of the area
    back = _frame([[0, 0, 1], [0, 4, 1], [4, 0, 1]], [[0, 1, 2]], 5, 5, dtype=dtype)
    assert np.array_equal(back.face_id, fr.face_id)
    # background and shading: light along the view axis, the face normal too -> intensity 1, the base colour itself
    assert np.all(fr.rgb[~want] == 255)
    assert np.all(fr.rgb[want] == [128, 64, 255])          # floor(255 c + 0.5): 128, 64.25 -> 64, 255.5 -> clamped


def test_depth_is_perspective_correct():
    # a plane Z = 1 + X through three corners; the ray of the pixel centre (x, y) meets it where Z = 1 / (1 - x)
    v = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 2.0], [0.0, 1.0, 1.0]])      # projects to (0, 0), (0.5, 0), (0, 1)
    fr = RR.raster_frame(v.astype(np.float32), np.array([[0, 1, 2]]), EYE3, ZERO3, 8.0, 8.0, 0.0, 0.0, 0.05, 8, 8)
    assert fr.covered.sum() > 5
    ii, jj = np.nonzero(fr.covered)
    x = (jj + 0.5) / 8.0
    assert np.allclose(fr.depth[ii, jj], 1.0 / (1.0 - x), rtol=1e-12, atol=0)


def test_overlapping_triangles_resolve_by_depth_and_ties_by_the_lower_id():
    near_tri = [[0, 0, 1], [4, 0, 1], [0, 4, 1]]
    far_tri = [[0, 0, 2], [8, 0, 2], [0, 8, 2]]          # projects onto the same pixels, twice as far
    v = far_tri + near_tri
    fr = _frame(v, [[0, 1, 2], [3, 4, 5]], 5, 5)
    assert np.all(fr.face_id[fr.covered] == 1) and np.all(fr.depth[fr.covered] == 1.0) and fr.covered.sum() == 10
    fr = _frame(v, [[3, 4, 5], [0, 1, 2]], 5, 5)
    assert np.all(fr.face_id[fr.covered] == 0)
    # the same triangle twice: an exact tie of the depth at every pixel goes to the lower id, in either order of vertices
    tie = _frame(near_tri + near_tri, [[3, 4, 5], [0, 1, 2]], 5, 5)
    assert np.all(tie.face_id[tie.covered] == 0) and tie.covered.sum() == 10
    assert np.all(tie.ambiguous[tie.covered])            # second-nearest at the same depth


def test_a_face_crossing_near_is_dropped_whole_and_a_degenerate_face_is_skipped():
    fr = _frame([[0, 0, 1], [4, 0, 1], [0, 4, 0.04]], [[0, 1, 2]], 5, 5, near=0.05)
    assert not fr.covered.any() and fr.n_near_dropped == 1 and np.all(fr.face_id == -1)
    fr = _frame([[0, 0, 1], [4, 0, 1], [0, 4, 0.05]], [[0, 1, 2]], 5, 5, near=0.05)      # Z == near: dropped as well
    assert not fr.covered.any()
    fr = _frame([[0.5, 0.5, 1], [2.5, 2.5, 1], [4.5, 4.5, 1]], [[0, 1, 2]], 5, 5)          # area exactly 0, through centres
    assert not fr.covered.any() and np.all(fr.rgb == 255)
    fr = _frame([[-9, -9, 1], [-5, -9, 1], [-9, -5, 1]], [[0, 1, 2]], 5, 5)                # bounding box misses the image
    assert not fr.covered.any() and fr.n_small == 0 and fr.n_large == 0


# ---- the conditions of the GPU scenes -------------------------------------------------------------------------------
@pytest.mark.parametrize('scene', RR.SCENES, ids=[s.name for s in RR.SCENES])
def test_scene_conditions(scene):
    """What tests/test_render.py assumes of its scenes, on the oracle's float64 body model: the ambiguous pixels are at
    most 2 % of the covered ones at V = 160 and 10 % at V = 6890 (caps: conditions of the scenes, not measurements),
    float32 and float64 agree on every other pixel, and every scene shows what it is there for."""
    model = synthetic.make_model(nu=scene.nu, nv=scene.nv)
    bm = R.BodyModelTensors(model, dtype=torch.float64)
    root, body, betas = (torch.from_numpy(a).double() for a in RR.scene_inputs(scene))
    vertices = R.smpl_fk(bm, body, betas, root)[0].numpy().astype(np.float32)
    assert vertices.shape == (scene.T, scene.nu * scene.nv, 3)
    f64 = RR.reference_frames(scene, vertices, model['f'])
    f32 = RR.reference_frames(scene, vertices, model['f'], dtype=np.float32)
    cam = RR.scene_camera(scene)
    for k, (a, b) in enumerate(zip(f64, f32)):
        share = a.ambiguous.sum() / float(a.covered.sum())
        print('{} frame {}: covered {}, ambiguous {} ({:.2f} %), small / large / near-dropped faces {} / {} / {}'
              .format(scene.name, k, a.covered.sum(), a.ambiguous.sum(), 100 * share, a.n_small, a.n_large,
                      a.n_near_dropped))
        assert a.covered.sum() >= 300
        assert share <= scene.cap
        clear = ~a.ambiguous
        assert np.array_equal(a.face_id[clear], b.face_id[clear])
        # no vertex so close to the near plane that the two precisions could drop different faces
        Rk, tk = (cam.R[k], cam.t[k]) if cam.R.ndim == 3 else (cam.R, cam.t)
        proj = RR.project(vertices[k], Rk, tk, cam.fx, cam.fy, cam.cx, cam.cy, np.float64)
        assert np.abs(proj[:, 2] - cam.near).min() > 1e-4
        if scene.name == 'crosses_near':
            assert a.n_near_dropped >= 10 and a.n_large >= 10 and a.n_small >= 10
        else:
            assert a.n_near_dropped == 0 and a.n_small >= 200
        if scene.name == 'leaves_image':
            assert (proj[:, 0] > scene.W).sum() >= 10 and a.covered[:, -1].any()
    if scene.name == 'three_frames':
        assert sum(a.n_large for a in f64) >= 5      # both paths of the raster kernel inside one launch


# ---- the C entry point without a GPU --------------------------------------------------------------------------------
def _desc(keep, **change):
    """A descriptor every check accepts; the pointers are host memory that a refused call never reads."""
    T, V, F, H_, W_ = 2, 16, 4, 8, 12
    buf = np.zeros(4096, np.float32)
    faces = np.array([[0, 1, 2], [2, 3, 4], [4, 5, 6], [13, 14, 15]], np.int32)
    keep += [buf, faces]
    p = ctypes.c_void_p(buf.ctypes.data)
    d = _lib.RenderDesc()
    d.T, d.V, d.n_faces, d.H, d.W = T, V, F, H_, W_
    d.vertices, d.faces, d.faces_host, d.normals, d.colors = p, p, _lib.iptr(faces), p, p
    d.color_mode, d.cam_R, d.cam_t, d.camera_per_frame = _lib.RENDER_COLOR_VERTEX, p, p, 0
    d.fx, d.fy, d.cx, d.cy, d.near = 10.0, 10.0, 6.0, 4.0, 0.05
    d.light[:], d.ambient, d.background[:] = (0.0, 0.0, -1.0), 0.3, (1.0, 1.0, 1.0)
    d.slab_frames = 0
    d.rgb, d.face_id, d.depth = p, p, p
    for k, v in change.items():
        if k == 'face':
            faces[v[0], v[1]] = v[2]
        elif k in ('light', 'background'):
            getattr(d, k)[:] = v
        else:
            setattr(d, k, v)
    return d, p


_up = lambda n: -(-n // 256) * 256      # the workspace is carved in pieces of 256 bytes


def test_bad_render_descriptors_are_refused_without_a_gpu():
    lib = _lib.lib()
    keep = []
    nbytes = lib.empose_render_workspace_bytes(2, 16, 8, 12)
    assert nbytes == _up(2 * 16 * 3 * 4) + _up(2 * 8 * 12 * 8)        # projected vertices and keys of one slab

    def call(ws_size=None, ws=True, **change):
        d, p = _desc(keep, **change)
        return lib.empose_render_meshes(ctypes.byref(d), p if ws else None, ctypes.c_size_t(nbytes if ws_size is None
                                                                                            else ws_size), None)
    assert lib.empose_render_meshes(None, None, 0, None) == EMPOSE_EINVAL
    for name in ('vertices', 'faces', 'colors', 'cam_R', 'cam_t', 'rgb'):
        assert call(**{name: None}) == EMPOSE_EINVAL, name
        assert b'null' in lib.empose_last_error()
    for name in ('T', 'V', 'n_faces', 'H', 'W'):
        for bad in (0, -3):
            assert call(**{name: bad}) == EMPOSE_EINVAL, name
    assert call(H=_lib.RENDER_MAX_IMAGE + 1) == EMPOSE_EINVAL and b'cap' in lib.empose_last_error()
    assert call(W=_lib.RENDER_MAX_IMAGE + 1) == EMPOSE_EINVAL
    for bad in (0.0, -0.05, float('nan'), float('inf')):
        assert call(near=bad) == EMPOSE_EINVAL and b'near' in lib.empose_last_error()
    assert call(color_mode=3) == EMPOSE_EINVAL and call(color_mode=-1) == EMPOSE_EINVAL
    assert call(ambient=1.5) == EMPOSE_EINVAL and call(ambient=-0.1) == EMPOSE_EINVAL
    assert call(light=(0.0, 0.0, 0.0)) == EMPOSE_EINVAL and call(light=(float('nan'), 0.0, 1.0)) == EMPOSE_EINVAL
    assert call(background=(float('inf'), 0.0, 0.0)) == EMPOSE_EINVAL
    assert call(fx=0.0) == EMPOSE_EINVAL and call(fy=float('nan')) == EMPOSE_EINVAL and call(cx=float('inf')) == EMPOSE_EINVAL
    assert call(slab_frames=-1) == EMPOSE_EINVAL
    assert call(face=(3, 2, 16)) == EMPOSE_EINVAL and b'face 3' in lib.empose_last_error()       # index == V
    assert call(face=(0, 0, -1)) == EMPOSE_EINVAL and b'face 0' in lib.empose_last_error()
    assert call(ws=False) == EMPOSE_EINVAL
    assert call(ws_size=nbytes - 1) == EMPOSE_EINVAL and b'workspace' in lib.empose_last_error()


def test_render_workspace_query():
    lib = _lib.lib()
    for T, V, H_, W_ in ((0, 16, 8, 8), (2, 0, 8, 8), (2, 16, 0, 8), (2, 16, 8, -1), (-1, 16, 8, 8),
                         (2, 16, _lib.RENDER_MAX_IMAGE + 1, 8), (2, 16, 8, _lib.RENDER_MAX_IMAGE + 1)):
        assert lib.empose_render_workspace_bytes(T, V, H_, W_) == 0
    # slabs of frames: bounded whatever T is
    big = lib.empose_render_workspace_bytes(10 ** 6, 6890, 512, 512)
    assert 0 < big <= (64 << 20) + 512 and big == lib.empose_render_workspace_bytes(10 ** 5, 6890, 512, 512)
    # one frame of the largest image needs more than the slab budget, and gets it
    assert lib.empose_render_workspace_bytes(7, 6890, 2048, 2048) == _up(6890 * 12) + 2048 * 2048 * 8


def test_render_desc_matches_the_header_field_order():
    text = open(os.path.join(ROOT, 'include', 'empose_hip.h')).read()
    end = re.search(r'\}\s*empose_render_desc;', text).start()
    body = text[text.rfind('typedef struct {', 0, end) + len('typedef struct {'):end]
    names = []
    for decl in re.sub(r'/\*.*?\*/', '', body, flags=re.S).split(';'):
        for part in decl.strip().split(','):
            if part.strip():
                names.append(re.findall(r'([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[[^\]]*\])*\s*$', part.strip())[0])
    assert names == [f[0] for f in _lib.RenderDesc._fields_]
    assert str(_lib.RENDER_MAX_IMAGE) in re.search(r'#define EMPOSE_RENDER_MAX_IMAGE (\d+)', text).group(1)


def test_cpu_tensors_raise():
    from em_pose_amd.bodymodels.smpl import SMPLLayer
    from em_pose_amd.vis import MeshRenderer
    layer = SMPLLayer(H.small_model())
    cam = CAM.pinhole(32, 24)._replace(t=np.array([0.0, 0.0, 3.0]))
    r = MeshRenderer(layer, 32, 24, camera=cam)
    V = layer.n_vertices
    with pytest.raises(_lib.EmposeError):
        r.render(torch.zeros(1, V, 3))
    with pytest.raises(_lib.EmposeError):
        r.render_bodies(torch.zeros(1, 63), torch.zeros(1, 10))
    with pytest.raises(ValueError):
        MeshRenderer(layer, _lib.RENDER_MAX_IMAGE + 1, 24)


# ---- cameras --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('eye, target, up', [((0.6, 0.3, 2.6), (0.0, -0.2, 0.0), (0, 1, 0)),
                                             ((-2.0, 1.5, -0.5), (0.1, 0.2, 0.3), (0, 1, 0)),
                                             ((0.0, 0.0, 3.0), (0.0, 0.0, 0.0), (0.3, 1.0, 0.2))])
def test_look_at_is_orthonormal_right_handed_and_looks_at_the_target(eye, target, up):
    R_, t = CAM.look_at(eye, target, up)
    assert np.allclose(R_ @ R_.T, np.eye(3), atol=1e-14) and abs(np.linalg.det(R_) - 1.0) < 1e-14
    assert np.allclose(np.cross(R_[0], R_[1]), R_[2], atol=1e-14)
    assert np.allclose(R_ @ np.asarray(eye) + t, 0.0, atol=1e-14)
    pc = R_ @ np.asarray(target, dtype=float) + t
    assert np.allclose(pc[:2], 0.0, atol=1e-14) and pc[2] > 0          # on the optical axis, in front
    above = R_ @ (np.asarray(target, dtype=float) + 0.1 * np.asarray(up, dtype=float)) + t
    assert above[1] < 0                                                 # image y points down


def test_pinhole_and_fit_camera_keep_every_joint_inside_the_image():
    cam = CAM.pinhole(160, 120, fov_y_deg=40.0)
    assert cam.cx == 80.0 and cam.cy == 60.0 and cam.fx == cam.fy
    assert np.isclose(np.rad2deg(2 * np.arctan(60.0 / cam.fy)), 40.0)
    rng = np.random.default_rng(3)
    for W_, H_, margin in ((160, 120, 0.15), (48, 64, 0.0), (131, 97, 0.3)):
        joints = rng.normal(0.0, 0.5, size=(40, 22, 3)) * [0.5, 1.0, 0.3] + rng.normal(0, 2.0, size=3)
        cam = CAM.fit_camera(torch.from_numpy(joints), W_, H_, margin=margin)
        xyz = CAM.project(cam, joints).reshape(-1, 3)
        assert xyz[:, 2].min() > cam.near
        assert np.all(np.abs(xyz[:, 0] - W_ / 2.0) <= (1 - margin) * W_ / 2.0 * (1 + 1e-6))
        assert np.all(np.abs(xyz[:, 1] - H_ / 2.0) <= (1 - margin) * H_ / 2.0 * (1 + 1e-6))
        # as close as the bound allows: some joint sits on the shrunk frame (or on the near bound)
        rel = np.maximum(np.abs(xyz[:, 0] - W_ / 2.0) / ((1 - margin) * W_ / 2.0),
                         np.abs(xyz[:, 1] - H_ / 2.0) / ((1 - margin) * H_ / 2.0))
        assert rel.max() > 0.999
        R_ = np.asarray(cam.R)
        assert np.allclose(R_ @ R_.T, np.eye(3), atol=1e-12)
    with pytest.raises(ValueError):
        CAM.fit_camera(np.zeros((0, 3)), 10, 10)


# ---- image output ---------------------------------------------------------------------------------------------------
def test_save_frames_and_contact_sheet(tmp_path, monkeypatch):
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, size=(3, 5, 7, 3), dtype=np.uint8)
    paths = VIO.save_frames(str(tmp_path / 'a'), torch.from_numpy(rgb), start=10, step=10)
    assert [os.path.basename(p).split('.')[0] for p in paths] == ['frame_000010', 'frame_000020', 'frame_000030']
    assert all(os.path.getsize(p) > 0 for p in paths)
    monkeypatch.setattr(VIO, '_pil', lambda: None)          # without PIL: binary PPM, standard library alone
    paths = VIO.save_frames(str(tmp_path / 'b'), rgb)
    assert all(p.endswith('.ppm') for p in paths)
    raw = open(paths[1], 'rb').read()
    assert raw.startswith(b'P6\n7 5\n255\n') and raw[len(b'P6\n7 5\n255\n'):] == rgb[1].tobytes()
    sheet = VIO.contact_sheet(list(rgb), columns=2)
    assert sheet.shape == (10, 14, 3) and np.array_equal(sheet[5:, :7], rgb[2]) and np.all(sheet[5:, 7:] == 255)
    assert np.array_equal(sheet[:5, 7:], rgb[1])
    assert VIO.side_by_side(rgb, rgb).shape == (3, 5, 14, 3)
    with pytest.raises(ValueError):
        VIO.save_frames(str(tmp_path / 'c'), rgb.astype(np.float32))
