"""
The HIP overlay ray caster (em_pose_amd/vis draw_primitives -> empose_render_overlay, csrc/overlay.hip) against the float64
restatement of its definition (tests/overlay_ref.py), on the scenes whose conditions tests/test_overlay_cpu.py checks on
the CPU.  The bodies are posed through SMPLLayer.forward on the device; the overlay of a frame (skeleton, sensor tripods,
residuals: about 170 primitives) is built from its joints by the builders of em_pose_amd/vis/overlay.py; the reference
evaluates the same float32 primitives at every pixel in float64 -- it has no screen boxes, so a box of the kernels that is
too small shows as a difference -- and once more in float32 as the control.

Per scene:
  prim_id     equal to the float64 reference at EVERY pixel outside the frame's ambiguity mask, background included;
  prim_depth  largest relative error at most 4 x the float32 control's largest of the scene + 1e-7 (printed before the assert);
  rgb         within one 8-bit level outside the mask, drawn over the rendered mesh with no mesh depth, with the mesh's own
              depth and alpha = 0, 0.5 and 1.  With a mesh depth, pixels where the hit lies within the mask's own depth
              tolerance (1e-4 relative) of the mesh are left out as well: there float32 may decide "in front" otherwise.

Measured on an MI355X: no id differs outside the mask in any scene; the kernels' depth error EQUALS the control's in every
scene (1.0e-7 three_frames, 1.5e-7 camera_per_frame, 2.1e-7 partial_tiles, 2.5e-7 one_frame, 3.3e-7 leaves_image, 3.5e-7
close_up, 1.3e-6 wide_angle), since the restatement follows them operation by operation; the largest rgb difference is 0
in every scene and variant.
"""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from em_pose_amd import synthetic
from em_pose_amd.bodymodels import tables as TB
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.vis import MeshRenderer, Primitives, draw_primitives
from em_pose_amd.vis.camera import Camera
from tests import overlay_ref as OR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {s.name: s for s in OR.SCENES}
VARIANTS = {'no_depth': (False, 0.0), 'alpha_0': (True, 0.0), 'alpha_half': (True, 0.5), 'alpha_1': (True, 1.0)}
_cache = {}


def _layer():
    if 'layer' not in _cache:
        model = synthetic.make_model(nu=OR.NU, nv=OR.NV)
        _cache['layer'] = (model, SMPLLayer(model).to(DEV))
    return _cache['layer']


def _to_dev(prims):
    return Primitives(prims.a.to(DEV), prims.b.to(DEV), prims.radius.to(DEV), prims.colors.to(DEV))


def _posed(scene):
    """The scene's bodies through SMPLLayer.forward, rendered, and the overlay of their joints, on the device."""
    key = ('posed', scene.name)
    if key not in _cache:
        model, layer = _layer()
        root, body, betas = (torch.from_numpy(a).to(DEV) for a in OR.scene_inputs(scene))
        with torch.no_grad():
            vertices, joints = layer(poses_body=body, betas=betas, poses_root=root)
        cam = OR.scene_camera(scene)
        renderer = MeshRenderer(layer, scene.W, scene.H, camera=cam)
        rgb, _, depth = renderer.render(vertices, return_buffers=True)
        host = OR.scene_primitives(scene, joints.cpu().numpy(), TB.model_parents(model))
        _cache[key] = dict(layer=layer, renderer=renderer, vertices=vertices.contiguous(), cam=cam, rgb=rgb, depth=depth,
                           host=host, prims=_to_dev(host))
    return _cache[key]


def _reference(scene):
    """Float64 frames with every variant's occlusion, and the float32 control's ids and depths; computed once."""
    key = ('ref', scene.name)
    if key not in _cache:
        p = _posed(scene)
        depth = p['depth'].cpu().numpy()
        variants = {name: dict(mesh_depth=depth if with_depth else None, hidden_alpha=alpha)
                    for name, (with_depth, alpha) in VARIANTS.items()}
        f64 = OR.reference_frames(scene, p['host'], rgb_in=p['rgb'].cpu().numpy(), variants=variants)
        f32 = OR.reference_frames(scene, p['host'], dtype=np.float32, ambiguity=False)
        _cache[key] = (f64, f32, depth)
    return _cache[key]


def _draw(p, name, **kw):
    with_depth, alpha = VARIANTS[name]
    return draw_primitives(p['rgb'].clone(), p['prims'], p['cam'], depth=p['depth'] if with_depth else None,
                           hidden_alpha=alpha, return_buffers=True, **kw)


@pytest.mark.parametrize('scene', OR.SCENES, ids=[s.name for s in OR.SCENES])
def test_scene_matches_the_float64_reference(scene):
    p = _posed(scene)
    f64, f32, mesh_depth = _reference(scene)
    first = None
    for name, (with_depth, alpha) in VARIANTS.items():
        rgb, prim_id, prim_depth = _draw(p, name)
        assert rgb.shape == (scene.T, scene.H, scene.W, 3) and rgb.dtype == torch.uint8 and rgb.is_cuda
        assert prim_id.dtype == torch.int32 and prim_depth.dtype == torch.float32
        rgb, prim_id, prim_depth = rgb.cpu().numpy(), prim_id.cpu().numpy(), prim_depth.cpu().numpy()
        if first is None:
            first = (prim_id, prim_depth)
        else:       # the mesh changes neither which primitive is nearest nor how far it is
            assert np.array_equal(prim_id, first[0])
            assert np.array_equal(prim_depth.view(np.uint32), first[1].view(np.uint32))
        worst, control, worst_rgb, wrong, shares = 0.0, 0.0, 0, 0, []
        for k in range(scene.T):
            a, b = f64[k], f32[k]
            clear = ~a.ambiguous
            shares.append(100.0 * a.ambiguous.sum() / float((a.covered | a.ambiguous).sum()))
            wrong += int((prim_id[k][clear] != a.prim_id[clear]).sum())
            hit = clear & a.covered & (prim_id[k] == a.prim_id)
            if hit.any():
                worst = max(worst, float(np.max(np.abs(prim_depth[k][hit].astype(np.float64) - a.prim_depth[hit])
                                                / a.prim_depth[hit])))
            ctl = clear & a.covered & (b.prim_id == a.prim_id)
            control = max(control, float(np.max(np.abs(b.prim_depth[ctl].astype(np.float64) - a.prim_depth[ctl])
                                                / a.prim_depth[ctl])))
            assert np.all(np.isinf(prim_depth[k][prim_id[k] < 0])) and np.all(prim_depth[k][prim_id[k] < 0] > 0)
            assert np.all(np.isfinite(prim_depth[k][prim_id[k] >= 0]))
            ok = clear & (prim_id[k] == a.prim_id)
            if with_depth:
                with np.errstate(invalid='ignore'):
                    ok &= ~(a.covered & (np.abs(a.prim_depth - mesh_depth[k]) <= OR.DEPTH_TOL * a.prim_depth))
            worst_rgb = max(worst_rgb, int(np.abs(rgb[k][ok].astype(int) - a.rgb[name][ok].astype(int)).max()))
        print('{} {}: mask shares {} %, ids that differ outside the mask {}, depth rel. error {:.3e} (control {:.3e}, bar '
              '{:.3e}), largest rgb difference {}'.format(scene.name, name, ['%.2f' % s for s in shares], wrong, worst,
                                                          control, 4 * control + 1e-7, worst_rgb))
        assert wrong == 0
        assert worst <= 4 * control + 1e-7
        assert worst_rgb <= 1


# ---- exact small cases ------------------------------------------------------------------------------------------------
# Identity camera with fx = fy = 8 and cx = cy = 4.5 on 9 x 9 pixels: the centre of pixel (4, 4) is the optical axis.
AXIS_CAM = Camera(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), 8.0, 8.0, 4.5, 4.5, 0.05)
COLOR = (0.5, 0.25, 1.0)


def _small(a, b, r, cam=AXIS_CAM, H_=9, W_=9, rgb_in=None, depth=None, alpha=0.0, colors=None):
    """One frame through the kernels and through the float64 reference: (rgb, prim_id, prim_depth) as arrays, Frame."""
    a, b, r = np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(r, np.float32)
    colors = np.tile(np.asarray([COLOR], np.float32), (len(r), 1)) if colors is None else np.asarray(colors, np.float32)
    rgb_in = np.full((H_, W_, 3), 255, np.uint8) if rgb_in is None else rgb_in
    prims = Primitives(torch.from_numpy(a)[None].to(DEV), torch.from_numpy(b)[None].to(DEV), torch.from_numpy(r).to(DEV),
                       torch.from_numpy(colors).to(DEV))
    out = draw_primitives(torch.from_numpy(rgb_in)[None].to(DEV).contiguous(), prims, cam,
                          depth=None if depth is None else torch.from_numpy(depth)[None].to(DEV), hidden_alpha=alpha,
                          return_buffers=True)
    want = OR.overlay_frame(a, b, r, colors, cam.R, cam.t, cam.fx, cam.fy, cam.cx, cam.cy, cam.near, H_, W_, rgb_in=rgb_in,
                            mesh_depth=depth, hidden_alpha=alpha)
    return tuple(x[0].cpu().numpy() for x in out), want


def _same_outside_the_mask(got, want, name):
    """Ids equal, depth within 2e-5 relative (the cap tests/test_overlay_cpu.py puts on float32 arithmetic of this
    definition), rgb within one level, outside the ambiguity mask and the band about the near plane."""
    rgb, prim_id, prim_depth = got
    clear = ~want.ambiguous & ~want.near_band
    assert np.array_equal(prim_id[clear], want.prim_id[clear]), name
    hit = clear & want.covered
    if hit.any():
        assert np.max(np.abs(prim_depth[hit] - want.prim_depth[hit]) / want.prim_depth[hit]) <= 2e-5, name
        assert np.abs(rgb[clear].astype(int) - want.rgb[clear].astype(int)).max() <= 1, name
    assert np.all(np.isinf(prim_depth[prim_id < 0]))


def test_hand_cases_bit_for_bit():
    # a sphere of radius 0.5 at Z = 2 on the ray of a pixel centre: its pole, exactly
    got, want = _small([[0, 0, 2]], [[0, 0, 2]], [0.5])
    assert got[2][4, 4] == 1.5 and got[1][4, 4] == 0 and want.prim_depth[4, 4] == 1.5
    assert np.all(got[0][4, 4] == [128, 64, 255])            # n = -z = the light: the base colour itself
    assert np.all(got[0][got[1] < 0] == 255)
    _same_outside_the_mask(got, want, 'sphere')
    # 40 identical spheres: id 0 wherever anything is hit, and the bits of the one sphere
    many, _ = _small([[0, 0, 2]] * 40, [[0, 0, 2]] * 40, [0.5] * 40)
    assert np.all(many[1][many[1] >= 0] == 0) and np.array_equal(many[1], got[1])
    assert np.array_equal(many[2].view(np.uint32), got[2].view(np.uint32)) and np.array_equal(many[0], got[0])
    # radius 0, a negative radius, a NaN endpoint, a NaN and an infinite radius: skipped
    skipped, _ = _small([[0, 0, 2], [0, 0, 1.5], [float('nan'), 0, 1], [0, 0, 1], [0, 0, 1], [0, 0, 2]],
                        [[0, 0, 2], [0, 0, 1.5], [0, 0, 1], [0, 0, 1], [0, float('inf'), 1], [0, 0, 2]],
                        [0.0, -0.5, 0.5, float('nan'), 0.5, 0.5])
    assert np.all(skipped[1][skipped[1] >= 0] == 5) and np.array_equal(skipped[1] >= 0, got[1] >= 0)
    assert np.array_equal(skipped[2].view(np.uint32), got[2].view(np.uint32)) and np.array_equal(skipped[0], got[0])
    # a sphere about the camera and one behind it cover nothing, and leave rgb alone
    rgb_in = np.random.default_rng(0).integers(0, 256, size=(9, 9, 3), dtype=np.uint8)
    none, _ = _small([[0, 0, 0], [0, 0, -2]], [[0, 0, 0], [0, 0, -2]], [0.5, 0.5], rgb_in=rgb_in)
    assert np.all(none[1] == -1) and np.all(np.isinf(none[2])) and np.array_equal(none[0], rgb_in)
    # a capsule through the near plane covers only pixels whose entry lies beyond it
    cam = AXIS_CAM._replace(near=0.75)
    got, want = _small([[-1, 0, 0.25]], [[1, 0, 1.25]], [0.125], cam=cam)
    assert (got[1] >= 0).any() and np.all(got[2][got[1] >= 0] > 0.75)
    assert np.all(got[1][4, 7:] == 0) and np.all(got[1][4, :3] == -1)
    _same_outside_the_mask(got, want, 'through near')
    # a capsule along the optical axis through a pixel centre: the side quadratic's leading coefficient is 0, the cap is hit
    got, want = _small([[0, 0, 2]], [[0, 0, 3]], [0.5])
    assert got[2][4, 4] == 1.5 and np.all(got[0][4, 4] == [128, 64, 255])
    _same_outside_the_mask(got, want, 'along the axis')
    # a == b against a capsule of length 1e-6: no difference outside the mask
    cam = Camera(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), 40.0, 40.0, 20.3, 18.6, 0.05)
    sphere, want = _small([[0.1, -0.05, 2]], [[0.1, -0.05, 2]], [0.6], cam=cam, H_=37, W_=41)
    short, _ = _small([[0.1, -0.05, 2]], [[0.1 + 1e-6, -0.05, 2]], [0.6], cam=cam, H_=37, W_=41)
    clear = ~want.ambiguous
    assert (sphere[1] >= 0).sum() > 300 and np.array_equal(sphere[1][clear], short[1][clear])
    hit = clear & (sphere[1] >= 0)
    assert np.max(np.abs(sphere[2][hit] - short[2][hit]) / sphere[2][hit]) <= 4e-5      # (two float32 results, 2e-5 each)
    assert np.abs(sphere[0][clear].astype(int) - short[0][clear].astype(int)).max() <= 1
    _same_outside_the_mask(sphere, want, 'sphere off axis')


def test_occlusion():
    rgb_in = np.random.default_rng(1).integers(0, 200, size=(9, 9, 3), dtype=np.uint8)
    depth2 = np.full((9, 9), 2.0, np.float32)
    # poles at 1.5 (in front of the mesh at 2) and at exactly 2 (the tie goes to the mesh)
    front, _ = _small([[0, 0, 2]], [[0, 0, 2]], [0.5], rgb_in=rgb_in, depth=depth2)
    plain, _ = _small([[0, 0, 2]], [[0, 0, 2]], [0.5], rgb_in=rgb_in)
    assert front[2][4, 4] == 1.5 and np.array_equal(front[0][4, 4], plain[0][4, 4]) and np.all(plain[0][4, 4] == [128, 64, 255])
    tie, want = _small([[0, 0, 2.5]], [[0, 0, 2.5]], [0.5], rgb_in=rgb_in, depth=depth2)
    assert tie[2][4, 4] == 2.0 and tie[1][4, 4] == 0 and np.array_equal(tie[0][4, 4], rgb_in[4, 4])
    # alpha = 0 behind the mesh everywhere: the bytes stay; ids and depths do not depend on the mesh
    assert np.array_equal(tie[0], rgb_in) and (tie[1] >= 0).sum() > 1
    # alpha = 1 is the call without a mesh depth; +inf hides nothing
    two = dict(a=[[0, 0, 2], [0.5, 0, 2.5]], b=[[0, 0, 2], [0.5, 0, 2.5]], r=[0.5, 0.5])
    plain, want = _small(two['a'], two['b'], two['r'], rgb_in=rgb_in)
    for kw in (dict(depth=depth2, alpha=1.0), dict(depth=np.full((9, 9), np.inf, np.float32))):
        got, _ = _small(two['a'], two['b'], two['r'], rgb_in=rgb_in, **kw)
        for x, y in zip(got, plain):
            assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y)
    # in between: visible pixels as without a mesh, hidden ones blended; against the reference
    half, want = _small(two['a'], two['b'], two['r'], rgb_in=rgb_in, depth=depth2, alpha=0.5)
    vis = (plain[1] >= 0) & (plain[2] < 2.0)
    hid = (plain[1] >= 0) & ~vis
    assert vis.any() and hid.any() and np.array_equal(half[0][vis], plain[0][vis]) and np.array_equal(half[0][plain[1] < 0], rgb_in[plain[1] < 0])
    assert np.any(half[0][hid] != plain[0][hid]) and np.any(half[0][hid] != rgb_in[hid])
    clear = ~want.ambiguous & ~(want.covered & (np.abs(want.prim_depth - 2.0) <= 2e-4))
    assert np.abs(half[0][clear].astype(int) - want.rgb[clear].astype(int)).max() <= 1


def test_culling_against_the_reference_without_boxes():
    cam = Camera(np.eye(3, dtype=np.float32), np.zeros(3, np.float32), 40.0, 40.0, 20.3, 18.6, 0.05)
    rng = np.random.default_rng(2)
    for P in (1, 257, 600):      # the only visible primitive is the last one: across the chunks of 256
        a = np.zeros((P, 3), np.float32)
        a[:, 0] = -50.0 - rng.uniform(0, 5, size=P)          # far off to the left: empty boxes
        a[:, 2] = 2.0
        b = a + rng.normal(0, 0.1, size=(P, 3)).astype(np.float32)
        r = np.full(P, 0.05, np.float32)
        r[::3] = 0.0                                         # ... or skipped
        a[-1], b[-1], r[-1] = (0.2, 0.1, 2.0), (-0.1, 0.3, 2.4), 0.3
        got, want = _small(a, b, r, cam=cam, H_=37, W_=41)
        assert np.all(want.prim_id[want.covered] == P - 1) and want.covered.sum() > 100
        _same_outside_the_mask(got, want, P)
    # a crowd where every chunk contributes survivors to every tile
    P = 600
    a = np.stack([rng.uniform(-0.5, 0.5, P), rng.uniform(-0.5, 0.5, P), rng.uniform(1.5, 3.0, P)], axis=1).astype(np.float32)
    b = a + rng.normal(0, 0.1, size=(P, 3)).astype(np.float32)
    got, want = _small(a, b, rng.uniform(0.01, 0.04, P).astype(np.float32), cam=cam, H_=37, W_=41,
                       colors=rng.uniform(0, 1, size=(P, 3)))
    assert len(np.unique(want.prim_id)) > 150 and (want.prim_id[~want.ambiguous] >= 256).any()
    _same_outside_the_mask(got, want, 'crowd')
    # one sphere over the whole image
    got, want = _small([[0.1, 0, 2]], [[0.1, 0, 2]], [1.5], cam=cam, H_=37, W_=41)
    assert want.covered.all() and np.all(got[1] == 0)
    _same_outside_the_mask(got, want, 'whole image')
    # (the wide-angle scene with primitives in the corners is test_scene_matches_the_float64_reference[wide_angle])


def test_a_second_call_gives_the_same_bits_and_a_frame_does_not_depend_on_its_batch():
    for scene in (BY_NAME['three_frames'], BY_NAME['camera_per_frame']):
        p = _posed(scene)
        batch = _draw(p, 'alpha_half')
        for x, y in zip(batch, _draw(p, 'alpha_half')):
            assert torch.equal(x, y)
        for slab in (2, 1):      # across a slab edge
            for x, y in zip(batch, _draw(p, 'alpha_half', slab_frames=slab)):
                assert torch.equal(x, y)
        cam = p['cam']
        for k in range(scene.T):      # ... and alone
            one = cam if np.ndim(cam.R) == 2 else cam._replace(R=cam.R[k:k + 1], t=cam.t[k:k + 1])
            alone = draw_primitives(p['rgb'][k:k + 1].clone(), p['prims'].frames(slice(k, k + 1)), one,
                                    depth=p['depth'][k:k + 1], hidden_alpha=0.5, return_buffers=True)
            for x, y in zip(batch, alone):
                assert torch.equal(x[k:k + 1], y)
            assert (alone[1] >= 0).sum() >= 50


# ---- the Python layer -------------------------------------------------------------------------------------------------
def test_render_with_overlays_is_render_then_draw_primitives():
    scene = BY_NAME['three_frames']
    p = _posed(scene)
    r = p['renderer']
    for alpha in (0.0, 0.6):
        got = r.render(p['vertices'], overlays=p['prims'], hidden_alpha=alpha, return_buffers=True)
        rgb, face_id, depth = r.render(p['vertices'], return_buffers=True)
        draw_primitives(rgb, p['prims'], p['cam'], depth=depth, hidden_alpha=alpha, light=r.light, ambient=r.ambient)
        for x, y in zip(got, (rgb, face_id, depth)):
            assert torch.equal(x, y)
        assert torch.equal(r.render(p['vertices'], overlays=[p['prims']], hidden_alpha=alpha), rgb)
        assert not torch.equal(rgb, p['rgb'])
    assert torch.equal(r.render(p['vertices'], overlays=None), p['rgb'])          # today's render, byte for byte
    assert torch.equal(r.render(p['vertices']), p['rgb'])
    root, body, betas = (torch.from_numpy(a).to(DEV) for a in OR.scene_inputs(scene))
    bodies = r.render_bodies(body, betas, poses_root=root, overlays=p['prims'], hidden_alpha=0.6)
    assert torch.equal(bodies, r.render(p['vertices'], overlays=p['prims'], hidden_alpha=0.6))


def _load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, 'scripts', name + '.py'))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_visualize_sensors_draws_the_readings_where_the_ground_truth_body_has_its_sensors():
    """The readings `--visualize_sensors` draws (vis.compare.sensor_overlays on the batch evaluate_real.py makes of a
    synthetic recording) lie within 0.15 m of the ground-truth body's virtual sensors -- offsets of a few centimetres --
    at every unmasked sensor, in the frame of the body that is shown; a mixed-up frame gives metres."""
    from em_pose_amd.data.data import RealSample
    from em_pose_amd.data.virtual_sensors import VirtualMarkerHelper
    from em_pose_amd.helpers.configuration import lgd_config
    from em_pose_amd.nn.models import create_model
    from em_pose_amd.vis.compare import sensor_overlays
    ev = _load_script('evaluate_real')
    device = torch.device(DEV)
    model = synthetic.make_model()
    torch.manual_seed(7)
    net = create_model(lgd_config(6, True, 2, lr=0.0005), SMPLLayer(model)).to(device).eval()
    smpl = SMPLLayer(model).to(device)
    d = synthetic.make_sequence(48, 103, ev._hip_sensors(net, device), missing_rate=0.05)
    sample = RealSample(str(d['id']), d['sensor_pos'], d['sensor_oris'], d['sensor_masks'].astype(np.float32),
                        d['smpl_poses'], d['smpl_shape'], d['smpl_trans'],
                        {'means': d['offset_means'], 'covs': d['offset_covs'], 'r': d['offset_r']})
    batch = ev.sample_to_batch(sample).to_gpu(device)
    masks = batch.marker_masks[0]
    assert 0 < int((masks == 0).sum()) < masks.numel() // 4
    poses = torch.cat([batch.poses_root[0], batch.poses_body[0]], dim=1).float()
    left, right = sensor_overlays(net, batch.marker_pos_real[0], batch.marker_ori_real[0], masks, poses,
                                  batch.shapes.reshape(1, -1), batch.offset_r.float(), batch.offset_t.float())
    readings = left[0]
    assert readings.n_frames == 48 and readings.n_primitives == 48 and len(right) == 3
    with torch.no_grad():
        v, _ = smpl(poses_body=batch.poses_body[0].float(), betas=batch.shapes.reshape(1, -1).float(),
                    poses_root=batch.poses_root[0].float())
        pos_gt, _, _ = VirtualMarkerHelper(smpl).get_virtual_pos_and_rot(v, net.vertex_ids)
    drawn = readings.radius[:, :12] > 0
    assert torch.equal(drawn, masks > 0)
    dist = (readings.a[:, :12] - pos_gt).norm(dim=-1)
    print('readings to ground-truth virtual sensors: largest distance {:.3f} m'.format(float(dist[drawn].max())))
    assert float(dist[drawn].max()) <= 0.15
    # the right half: the estimate's virtual sensors (here: of the ground-truth pose) and the residual capsules between
    residual = right[2]
    assert torch.equal(residual.a, readings.a[:, :12]) and torch.equal(residual.b, right[1].a[:, :12])
    # (the recording's own offsets scatter about the means the estimate is given: centimetres, not the frame's metres)
    assert float((residual.b - residual.a).norm(dim=-1)[drawn].max()) <= 0.15
    assert torch.equal(residual.radius > 0, drawn)


def _images(directory):
    out = []
    for name in sorted(os.listdir(directory)):
        path = os.path.join(directory, name)
        if name.endswith('.png'):
            from PIL import Image
            out.append(np.asarray(Image.open(path)))
        else:
            raw = open(path, 'rb').read()
            out.append(np.frombuffer(raw[len(b'P6\n64 48\n255\n'):], dtype=np.uint8).reshape(48, 64, 3))
    return out


def test_render_sequence_draws_skeleton_and_sensors(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
    cmd = [sys.executable, os.path.join(ROOT, 'scripts', 'render_sequence.py'), '--synthetic', '--frames', '4',
           '--width', '64', '--height', '48']
    dirs = [str(tmp_path / 'plain'), str(tmp_path / 'overlay')]
    runs = [subprocess.Popen(c, cwd=str(tmp_path), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             universal_newlines=True)
            for c in (cmd + ['--out', dirs[0]], cmd + ['--skeleton', '--sensors', '--out', dirs[1]])]
    done = [r.communicate(timeout=300) for r in runs]
    for r, (_, err) in zip(runs, done):
        assert r.returncode == 0, err[-3000:]
    plain, overlay = _images(dirs[0]), _images(dirs[1])
    assert len(plain) == len(overlay) == 4
    for x, y in zip(plain, overlay):
        assert x.shape == y.shape == (48, 64, 3) and (x != y).any(axis=-1).sum() >= 10
