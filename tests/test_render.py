"""
The HIP mesh renderer (em_pose_amd/vis MeshRenderer -> empose_render_meshes, csrc/raster.hip) against the float64
restatement of its definition (tests/raster_ref.py), on the scenes whose conditions tests/test_render_cpu.py checks on
the CPU.  The bodies are posed through SMPLLayer.forward on the device; the reference rasterises the same float32
vertices in float64, and once more in float32 as the control.

Per scene, for smooth shading, flat shading with per-vertex colours and smooth shading with per-frame colours:
  face_id  equal to the float64 reference at EVERY pixel outside the frame's ambiguity mask, background included;
  depth    largest relative error at most 4 x the float32 control's largest of the scene + 1e-7 (printed before the assert);
  rgb      within one 8-bit level (the rounding step of floor(255 c + 0.5)) outside the mask where the reference normal
           is not degenerate.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from em_pose_amd import synthetic
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.vis import MeshRenderer
from em_pose_amd.vis.camera import Camera
from tests import raster_ref as RR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {s.name: s for s in RR.SCENES}
_cache = {}


def _layer(nu, nv):
    key = ('layer', nu, nv)
    if key not in _cache:
        model = synthetic.make_model(nu=nu, nv=nv)
        _cache[key] = (model, SMPLLayer(model).to(DEV))
    return _cache[key]


def _posed(scene):
    """The scene's bodies through SMPLLayer.forward, their normals and two sets of colours, on the device."""
    key = ('posed', scene.name)
    if key not in _cache:
        model, layer = _layer(scene.nu, scene.nv)
        root, body, betas = (torch.from_numpy(a).to(DEV) for a in RR.scene_inputs(scene))
        with torch.no_grad():
            vertices, _ = layer(poses_body=body, betas=betas, poses_root=root)
            normals = layer.vertex_normals(vertices)
        rng = np.random.default_rng(scene.seed + 1000)
        V = vertices.shape[1]
        col_v = torch.from_numpy(rng.uniform(0.05, 1.0, size=(V, 3)).astype(np.float32)).to(DEV)
        col_f = torch.from_numpy(rng.uniform(0.05, 1.0, size=(scene.T, V, 3)).astype(np.float32)).to(DEV)
        _cache[key] = dict(model=model, layer=layer, inputs=(root, body, betas), vertices=vertices.contiguous(),
                           normals=normals.contiguous(), col_v=col_v, col_f=col_f)
    return _cache[key]


def _variants(p):
    return {'smooth': dict(normals=p['normals'], colors=None),
            'flat_vertex_colors': dict(normals='flat', colors=p['col_v']),
            'smooth_frame_colors': dict(normals=p['normals'], colors=p['col_f'])}


def _reference(scene):
    """Float64 frames with every variant's shading, and the float32 control's face ids and depths; computed once."""
    key = ('ref', scene.name)
    if key not in _cache:
        p = _posed(scene)
        host = lambda t: None if t is None or isinstance(t, str) else t.cpu().numpy()
        variants = {name: dict(normals=host(kw['normals']), colors=(0.7, 0.7, 0.7) if kw['colors'] is None
                               else host(kw['colors'])) for name, kw in _variants(p).items()}
        v = p['vertices'].cpu().numpy()
        f64 = RR.reference_frames(scene, v, p['model']['f'], variants=variants)
        f32 = RR.reference_frames(scene, v, p['model']['f'], dtype=np.float32)
        _cache[key] = (f64, f32)
    return _cache[key]


def _renderer(scene, layer):
    return MeshRenderer(layer, scene.W, scene.H, camera=RR.scene_camera(scene))


@pytest.mark.parametrize('scene', RR.SCENES, ids=[s.name for s in RR.SCENES])
def test_scene_matches_the_float64_reference(scene):
    p = _posed(scene)
    f64, f32 = _reference(scene)
    r = _renderer(scene, p['layer'])
    first = None
    for name, kw in _variants(p).items():
        rgb, face_id, depth = r.render(p['vertices'], normals=kw['normals'], colors=kw['colors'], return_buffers=True)
        assert rgb.shape == (scene.T, scene.H, scene.W, 3) and rgb.dtype == torch.uint8 and rgb.is_cuda
        assert face_id.dtype == torch.int32 and depth.dtype == torch.float32
        rgb, face_id, depth = rgb.cpu().numpy(), face_id.cpu().numpy(), depth.cpu().numpy()
        if first is None:
            first = (face_id, depth)
        else:       # the shading changes neither what is visible nor how far it is
            assert np.array_equal(face_id, first[0]) and np.array_equal(depth.view(np.uint32), first[1].view(np.uint32))
        worst, control, worst_rgb, wrong = 0.0, 0.0, 0, 0
        for k in range(scene.T):
            a, b = f64[k], f32[k]
            clear = ~a.ambiguous
            share = a.ambiguous.sum() / float(a.covered.sum())
            assert share <= scene.cap, 'the scene misses its condition on these vertices: {:.2f} %'.format(100 * share)
            wrong += int((face_id[k][clear] != a.face_id[clear]).sum())
            hit = clear & a.covered & (face_id[k] == a.face_id)
            if hit.any():
                worst = max(worst, float(np.max(np.abs(depth[k][hit].astype(np.float64) - a.depth[hit]) / a.depth[hit])))
            ctl = clear & a.covered & (b.face_id == a.face_id)
            control = max(control, float(np.max(np.abs(b.depth[ctl].astype(np.float64) - a.depth[ctl]) / a.depth[ctl])))
            assert np.all(np.isinf(depth[k][face_id[k] < 0])) and np.all(depth[k][face_id[k] < 0] > 0)
            assert np.all(np.isfinite(depth[k][face_id[k] >= 0]))
            ok = clear & a.normal_ok[name] & (face_id[k] == a.face_id)
            worst_rgb = max(worst_rgb, int(np.abs(rgb[k][ok].astype(int) - a.rgb[name][ok].astype(int)).max()))
        print('{} {}: face ids that differ outside the mask {}, depth rel. error {:.3e} (control {:.3e}, bar {:.3e}), '
              'largest rgb difference {}'.format(scene.name, name, wrong, worst, control, 4 * control + 1e-7, worst_rgb))
        assert wrong == 0
        assert worst <= 4 * control + 1e-7
        assert worst_rgb <= 1


class _Faces(object):
    """What MeshRenderer needs of a layer for flat shading: the faces."""

    def __init__(self, faces):
        self.faces = torch.tensor(faces, dtype=torch.int32)


def test_hand_cases_match_the_reference_exactly():
    """Small exact cases (every number a short binary fraction: float32 and float64 agree to the bit, so the ambiguity
    mask is not needed): a pixel centre exactly on an edge is covered, the nearer face wins whatever its id, an exact tie
    goes to the lower id whatever order the lanes arrive in, a face across the near plane is dropped whole, a face without
    area is skipped, and a face larger than a lane's share is walked by the wave with the same result."""
    cam = Camera(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), 1.0, 1.0, 0.0, 0.0, 0.05)
    near_tri, far_tri = [[0, 0, 1], [4, 0, 1], [0, 4, 1]], [[0, 0, 2], [8, 0, 2], [0, 8, 2]]
    big = [[0, 0, 1], [40, 0, 1], [0, 40, 1]]
    cases = [
        ('edge', near_tri, [[0, 1, 2]], 5, 5),
        ('far_first', far_tri + near_tri, [[0, 1, 2], [3, 4, 5]], 5, 5),
        ('near_first', far_tri + near_tri, [[3, 4, 5], [0, 1, 2]], 5, 5),
        ('tie', near_tri * 40, [[3 * k, 3 * k + 1, 3 * k + 2] for k in reversed(range(40))], 5, 5),
        ('crosses_near', [[0, 0, 1], [4, 0, 1], [0, 4, 0.03125]] + far_tri, [[0, 1, 2], [3, 4, 5]], 5, 5),
        ('degenerate', [[0.5, 0.5, 1], [2.5, 2.5, 1], [4.5, 4.5, 1]] + far_tri, [[0, 1, 2], [3, 4, 5]], 5, 5),
        ('wave', big + far_tri, [[0, 1, 2], [3, 4, 5]], 37, 41),
        ('wave_tie', big * 3, [[6, 7, 8], [0, 1, 2], [3, 4, 5]], 37, 41),
    ]
    for name, verts, faces, H_, W_ in cases:
        v = np.asarray(verts, dtype=np.float32)
        want = RR.raster_frame(v, faces, cam.R, cam.t, 1.0, 1.0, 0.0, 0.0, 0.05, H_, W_, colors=(0.5, 0.25, 1.0))
        r = MeshRenderer(_Faces(faces), W_, H_, camera=cam, color=(0.5, 0.25, 1.0))
        rgb, face_id, depth = r.render(torch.from_numpy(v)[None].to(DEV), normals='flat', return_buffers=True)
        assert np.array_equal(face_id[0].cpu().numpy(), want.face_id), name
        assert np.array_equal(depth[0].cpu().numpy().astype(np.float64), want.depth), name
        assert np.array_equal(rgb[0].cpu().numpy(), want.rgb), name
    assert want.n_large == 3 and (want.face_id == 0).sum() > 256      # (the last case went through the wave path)


def test_a_second_launch_gives_the_same_bits_and_a_frame_does_not_depend_on_its_batch():
    for scene in (BY_NAME['three_frames'], BY_NAME['camera_per_frame']):
        p = _posed(scene)
        r = _renderer(scene, p['layer'])
        kw = dict(normals=p['normals'], colors=p['col_f'], return_buffers=True)
        batch = r.render(p['vertices'], **kw)
        again = r.render(p['vertices'], **kw)
        for x, y in zip(batch, again):
            assert torch.equal(x, y)
        # ... across a slab edge: slabs of two frames cut the three apart, slabs of one frame everywhere
        for slab in (2, 1):
            r.slab_frames = slab
            for x, y in zip(batch, r.render(p['vertices'], **kw)):
                assert torch.equal(x, y)
        r.slab_frames = 0
        cam = r.camera
        for k in range(scene.T):      # ... and alone
            one = cam if np.ndim(cam.R) == 2 else cam._replace(R=cam.R[k:k + 1], t=cam.t[k:k + 1])
            alone = r.render(p['vertices'][k:k + 1], normals=p['normals'][k:k + 1], colors=p['col_f'][k:k + 1],
                             return_buffers=True, camera=one)
            for x, y in zip(batch, alone):
                assert torch.equal(x[k:k + 1], y)
            assert (alone[1] >= 0).sum() >= 300


def test_no_frames_give_empty_tensors():
    scene = BY_NAME['one_frame']
    p = _posed(scene)
    r = _renderer(scene, p['layer'])
    rgb, face_id, depth = r.render(p['vertices'][:0], return_buffers=True)
    assert rgb.shape == (0, scene.H, scene.W, 3) and rgb.dtype == torch.uint8 and rgb.is_cuda
    assert face_id.shape == (0, scene.H, scene.W) and depth.shape == (0, scene.H, scene.W)
    assert r.render(p['vertices'][:0]).shape == (0, scene.H, scene.W, 3)


def test_render_bodies_is_render_of_the_forwarded_mesh():
    scene = BY_NAME['three_frames']
    p = _posed(scene)
    r = _renderer(scene, p['layer'])
    root, body, betas = p['inputs']
    for shading in ('smooth', 'flat'):
        got = r.render_bodies(body, betas, poses_root=root, normals=shading, colors=p['col_v'], return_buffers=True)
        want = r.render(p['vertices'], normals=shading, colors=p['col_v'], return_buffers=True)
        for x, y in zip(got, want):
            assert torch.equal(x, y)
    # without a camera anywhere the first call fits one to its joints: the body is in view
    auto = MeshRenderer(p['layer'], scene.W, scene.H)
    _, face_id, _ = auto.render_bodies(body, betas, poses_root=root, return_buffers=True)
    assert auto.camera is not None and all((face_id[k] >= 0).sum() >= 300 for k in range(scene.T))
    from em_pose_amd.vis.camera import project
    xyz = project(auto.camera, p['layer'].fk_joints(body, betas, poses_root=root).cpu().numpy()).reshape(-1, 3)
    assert np.all((xyz[:, 0] > 0) & (xyz[:, 0] < scene.W) & (xyz[:, 1] > 0) & (xyz[:, 1] < scene.H))      # every joint in view


def _figures_masked(stdout):
    """stdout of evaluate_real.py with the two wall-clock figures of its throughput line replaced: they differ between
    any two runs of the same command; every other character is compared."""
    return re.sub(r'frames in [0-9.]+ s on (.*?): [0-9]+ frames/s', r'frames in <s> s on \1: <n> frames/s', stdout)


def test_evaluate_real_visualize_writes_the_frames_and_leaves_stdout_alone(tmp_path):
    """`--visualize 0` renders recording 0 (3460 frames, every 10th: 346 images) after the tables; stdout is that of the
    same command without the flag, character for character except the seconds and frames/s of the throughput line."""
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    cmd = [sys.executable, os.path.join(ROOT, 'scripts', 'evaluate_real.py'), '--synthetic', '--max_sequences', '2']
    out_dir = str(tmp_path / 'vis')
    runs = [subprocess.Popen(c, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             universal_newlines=True)
            for c in (cmd, cmd + ['--visualize', '0', '--visualize_dir', out_dir, '--visualize_size', '96'])]
    (plain_out, plain_err), (vis_out, vis_err) = [r.communicate(timeout=600) for r in runs]
    assert runs[0].returncode == 0, plain_err[-3000:]
    assert runs[1].returncode == 0, vis_err[-3000:]
    assert 'Overall average' in plain_out and 'frames/s' in plain_out
    assert _figures_masked(vis_out) == _figures_masked(plain_out)
    assert '<s>' in _figures_masked(plain_out)
    n = len(range(0, synthetic.README_SEQUENCE_LENGTHS[0], 10))
    files = sorted(os.listdir(out_dir))
    assert len(files) == n == 346
    assert files[0].startswith('frame_000000.') and files[-1].startswith('frame_003450.')
    assert '{} frames'.format(n) in vis_err and out_dir in vis_err and '--visualize' not in plain_err
    assert not os.path.exists(str(tmp_path / 'vis' / 'vis'))      # nothing went to the default ./vis/<recording id>
    # a frame is two panels side by side and shows two bodies on the background
    first = os.path.join(out_dir, files[0])
    if first.endswith('.png'):
        from PIL import Image
        img = np.asarray(Image.open(first))
    else:
        raw = open(first, 'rb').read()
        img = np.frombuffer(raw[len(b'P6\n192 96\n255\n'):], dtype=np.uint8).reshape(96, 192, 3)
    assert img.shape == (96, 192, 3)
    for half in (img[:, :96], img[:, 96:]):
        body_px = (half != 255).any(axis=-1).sum()
        assert 300 <= body_px < 96 * 96
