"""
Per-subject sensor offsets from calibration recordings in HIP (csrc/offset_stats.hip, em_pose_amd/data/offsets.py) on the
160-vertex body model: the per-frame offsets element by element against the float64 restatement
(tests/offset_estimation_ref.py) with the bar of tests/test_sample_sensors.py, the statistics against float64 with bounds
derived from the measured per-frame error, the shapes at which the two-pass reduction changes path, determinism and the
independence of a group from the rest of the batch, and the estimator end to end on noisy synthetic recordings, where
the bounds follow from the noise the test injects.

The bounds of the statistics, per (group, sensor) with n counting frames.  eps is the largest error of an element of
local_f against float64 in the same launch, eps_q the largest Frobenius error of a q_f; before a bound is derived from
them every launch's per-frame outputs are held to caps that do not depend on the kernel (_check_per_frame):
  means    |d| <= eps + 1e-7 |means64|: a mean of values each within eps, then the fp32 rounding of the output;
  covs     |d| <= 2 sigma eps' + eps'^2 + 1e-7 max|covs64|, eps' = eps sqrt(n / (n - 1)), sigma^2 the largest variance: with
           y the centred float64 samples and e the centred errors (sum e^2 <= n eps^2 per component), the difference is
           (sum y e^T + sum e y^T + sum e e^T) / (n - 1); Cauchy-Schwarz bounds a cross term by
           sqrt((n - 1) sigma^2) sqrt(n eps^2) / (n - 1) = sigma eps' and the last term by eps'^2; then the fp32
           rounding of the output;
  r        |d|_F <= 2 eps_q / (s2 + s3) + 1e-6: the perturbation bound of the orthogonal polar factor of the mean of Q
           (singular values s1 >= s2 >= s3 in float64), then the fp32 rounding of a matrix of unit scale;
  r_trace  |d| <= sqrt(3) eps_q + 4e-7: the sum of the singular values is sqrt(3)-Lipschitz in the Frobenius norm, then
           the fp32 rounding of a value of at most 3;
  counts   exact; n = 0 and n = 1 give the defined values exactly where they are defined to be zeros or the identity.
The bound of r needs a well-determined mean: the inputs have a few degrees of rotation noise, and every test asserts
s3 >= 0.5 on the float64 side.
"""
import types
import warnings

import numpy as np
import pytest
import torch

from em_pose_amd import synthetic
from em_pose_amd.bodymodels import tables as TB
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.data import offsets as OFS
from em_pose_amd.data.data import ABatch, RealSample
from em_pose_amd.data.transforms import SMPLFK, NormalizeRealMarkers, SampleMarkersWithOffsets
from em_pose_amd.data.virtual_sensors import VirtualMarkerHelper
from em_pose_amd.helpers.configuration import lgd_config
from tests import helpers as H
from tests import offset_estimation_ref as REF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
gpu = lambda a, dtype=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)
STATS = ('means', 'covs', 'r', 'r_trace', 'counts')


def _stub(faces):
    """What VirtualMarkerHelper reads of a body model: the faces."""
    return types.SimpleNamespace(model={'f': np.asarray(faces, dtype=np.int64)})


def _launch(faces, verts, ids, p, Rr, masks, groups, per_frame=True):
    out = OFS.offset_stats(VirtualMarkerHelper(_stub(faces)), gpu(verts), ids, gpu(p), gpu(Rr),
                           None if masks is None else gpu(masks), groups, per_frame=per_frame)
    return out


def _host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


# (first_frame, n_frames): 1, 2, 255, 0, 256, 257 and 513 frames, three frames of no group after the empty one
SHAPE_GROUPS = [(0, 1), (1, 2), (3, 255), (258, 0), (261, 256), (517, 257), (774, 513)]
T_ALL = 1300
# The per-frame comparison runs on the first 300 frames: a group inside one chunk, then one of a full chunk and a part.
FRAME_GROUPS = [(0, 40), (40, 260)]
T_FRAMES = 300
# Every sensor frame of the inputs is well conditioned, |nh x s| >= 0.5 in float64 (REF.posed_small; the recipe of
# tests/test_virtual_sensors_vjp.py, which uses 0.2): a frame amplifies the rounding of its vertices by 1 / |nh x s|, and
# the row bar compares two fp32 evaluations of it -- 4 x the control's error plus a floor of 1e-7 of the row's scale, about
# one rounding of a unit vector.  With the amplification at most 2 an fp32 frame stays near that floor however its
# products are contracted.  The bar remains a draw per row, because the control's own error varies tenfold from row to
# row: on the MI355X one of 1300 rows at |nh x s| >= 0.2 missed it with an error of 4e-7 of its scale.  So the row bar
# runs on the few hundred rows the paths of the kernel need (a seed change can still fail it without a bug: DESIGN.md
# section 9), and every launch is held by the caps of _check_per_frame, which are no draw.
MIN_CROSS = 0.5


def _layout_masks(name, rng, t, m):
    masks = (rng.uniform(size=(t, m)) > 0.05).astype(np.float32)
    if name == 'shapes':
        masks[:3] = 1.0                      # the groups of one and two frames count every sensor
        masks[774:1287, 3] = 0.0             # a sensor that is never read in its group
        masks[517:774, 5] = 0.0
        masks[517 + 100, 5] = 1.0            # a sensor that is read in exactly one frame
    return masks


@pytest.fixture(scope='module')
def scene():
    """1300 posed small-model meshes with noisy readings (5 mm, 2 degrees), and once for all layouts the per-frame
    offsets of every frame in float64 and in the float32 CPU control; then per layout its masks, groups, launch and
    float64 statistics.  The irregular five-sensor mesh is a scene of its own."""
    rng = np.random.default_rng(61)
    faces, ids = np.asarray(H.small_model()['f'], dtype=np.int64), REF.small_ids()
    verts = REF.posed_small(T_ALL, 62, ids=ids, min_cross=MIN_CROSS)
    p, Rr, t, r0 = REF.noisy_readings(verts, faces, ids, rng)
    o64, Q64 = REF.per_frame(verts, faces, ids, p, Rr, None, torch.float64)
    o32, Q32 = REF.per_frame(verts, faces, ids, p, Rr, None, torch.float32)
    layouts = {}
    for name, groups in (('frames', FRAME_GROUPS), ('two_groups', [(0, 700), (700, 600)]), ('shapes', SHAPE_GROUPS)):
        t = T_FRAMES if name == 'frames' else T_ALL
        masks = _layout_masks(name, rng, t, len(ids))
        layouts[name] = dict(faces=faces, verts=verts[:t], ids=ids, p=p[:t], Rr=Rr[:t], masks=masks, groups=groups,
                             o64=o64[:t], Q64=Q64[:t], o32=o32[:t], Q32=Q32[:t])
    pts, ifaces = REF.irregular_mesh()
    iverts = (pts[None] + rng.normal(0, 0.01, (40,) + pts.shape)).astype(np.float32)
    iids = [0, 11, 12, 1, 14]
    assert REF.min_cross_of(iverts, ifaces, iids).min() >= MIN_CROSS
    deg = np.bincount(ifaces.reshape(-1))[iids]
    assert deg.max() == 7 and len(set(deg.tolist())) > 2      # mixed degrees: max_deg 7 with shorter rows
    ip, iR, _, _ = REF.noisy_readings(iverts, ifaces, iids, rng, pos_noise=0.05)
    imasks = (rng.uniform(size=(40, 5)) > 0.1).astype(np.float32)
    o, Q = REF.per_frame(iverts, ifaces, iids, ip, iR, None, torch.float64)
    oc, Qc = REF.per_frame(iverts, ifaces, iids, ip, iR, None, torch.float32)
    layouts['irregular'] = dict(faces=ifaces, verts=iverts, ids=iids, p=ip, Rr=iR, masks=imasks, groups=[(0, 40)],
                                o64=o, Q64=Q, o32=oc, Q32=Qc)
    for name, L in layouts.items():
        counted = np.zeros(L['masks'].shape[0], bool)
        for first, n in L['groups']:
            counted[first:first + n] = True
        eff = L['masks'] * counted[:, None]           # zeros are expected where no group holds the frame, too
        L['eff'] = eff
        for k in ('o64', 'o32'):
            L[k] = L[k] * eff[..., None]
        for k in ('Q64', 'Q32'):
            L[k] = L[k] * eff[..., None, None]
        L['ref'] = REF.statistics(L['o64'], L['Q64'], L['masks'], L['groups'])
        L['got'] = _host(_launch(L['faces'], L['verts'], L['ids'], L['p'], L['Rr'], L['masks'], L['groups']))
        L['eps'] = float(np.abs(L['got']['local_frames'] - L['o64']).max())
        L['eps_q'] = float(np.sqrt(((L['got']['q_frames'] - L['Q64']) ** 2).sum(axis=(-1, -2))).max())
        print('{}: eps {:.3e} eps_q {:.3e}'.format(name, L['eps'], L['eps_q']))
    return layouts


def _check_statistics(name, got, ref, eps, eps_q):
    """The bounds of the module docstring for every (group, sensor); prints the largest ratio to each bound."""
    assert np.array_equal(got['counts'], ref['counts']), name
    worst = {'means': 0.0, 'covs': 0.0, 'r': 0.0, 'r_trace': 0.0}
    g_n, m_n = ref['counts'].shape
    for g in range(g_n):
        for m in range(m_n):
            n = int(ref['counts'][g, m])
            at = '{} group {} sensor {} n {}'.format(name, g, m, n)
            if n == 0:
                assert not got['means'][g, m].any() and not got['covs'][g, m].any(), at
                assert np.array_equal(got['r'][g, m], np.eye(3, dtype=np.float32)) and got['r_trace'][g, m] == 3.0, at
                continue
            s = ref['sing'][g, m]
            assert s[2] >= 0.5, at + ': the inputs must determine the mean rotation'
            d = np.abs(got['means'][g, m] - ref['means'][g, m])
            bound = eps + 1e-7 * np.abs(ref['means'][g, m])
            assert (d <= bound).all(), (at, 'means', d, bound)
            worst['means'] = max(worst['means'], float((d / bound).max()))
            if n == 1:
                assert not got['covs'][g, m].any(), at
            else:
                e1 = eps * np.sqrt(n / (n - 1.0))
                sigma = np.sqrt(np.diag(ref['covs'][g, m]).max())
                bound = 2 * sigma * e1 + e1 * e1 + 1e-7 * np.abs(ref['covs'][g, m]).max()
                d = np.abs(got['covs'][g, m] - ref['covs'][g, m]).max()
                assert d <= bound, (at, 'covs', d, bound)
                worst['covs'] = max(worst['covs'], float(d / bound))
            d = np.sqrt(((got['r'][g, m] - ref['r'][g, m]) ** 2).sum())
            bound = 2 * eps_q / (s[1] + s[2]) + 1e-6
            assert d <= bound, (at, 'r', d, bound)
            worst['r'] = max(worst['r'], float(d / bound))
            d = abs(got['r_trace'][g, m] - ref['r_trace'][g, m])
            bound = np.sqrt(3.0) * eps_q + 4e-7
            assert d <= bound, (at, 'r_trace', d, bound)
            worst['r_trace'] = max(worst['r_trace'], float(d / bound))
    print('{}: largest error as a fraction of its bound {}'.format(name, worst))


# ---- 1. per-frame outputs ---------------------------------------------------------------------------------------------------
def _check_per_frame(name, L):
    """What holds the per-frame outputs of EVERY launch before a bound is derived from their error, with caps that do not
    depend on the kernel: frames that do not count, or that no group holds, are exact zeros and nothing is NaN; the largest
    error of a row is at most 1e-4 x the row's scale (the first half of the row bar); and eps and eps_q, the largest
    errors of the launch, are at most 4 x the largest error of the float32 CPU control over the launch plus 1e-7 x the
    largest scale -- the second half of the row bar with its constants, taken over the launch instead of row by row,
    where it is a draw (see MIN_CROSS)."""
    got, off = L['got'], L['eff'] == 0
    assert off.any() and not got['local_frames'][off].any() and not got['q_frames'][off].any(), name
    assert np.isfinite(got['local_frames']).all() and np.isfinite(got['q_frames']).all(), name
    flat = lambda x: np.asarray(x, dtype=np.float64).reshape(x.shape[0], -1)
    for what, g, w64 in (('local_f', got['local_frames'], L['o64']), ('q_f', got['q_frames'], L['Q64'])):
        err, scale = np.abs(flat(g) - flat(w64)).max(axis=1), np.abs(flat(w64)).max(axis=1)
        assert (err <= 1e-4 * scale).all(), (name, what, int(np.argmax(err - 1e-4 * scale)))
    c_eps = float(np.abs(L['o32'] - L['o64']).max())
    c_eps_q = float(np.sqrt(((L['Q32'] - L['Q64']) ** 2).sum(axis=(-1, -2))).max())
    cap, cap_q = 4 * c_eps + 1e-7 * float(np.abs(L['o64']).max()), 4 * c_eps_q + 1e-7 * np.sqrt(3.0)     # |Q|_F = sqrt(3)
    print('{}: eps / cap {:.3f}, eps_q / cap {:.3f}'.format(name, L['eps'] / cap, L['eps_q'] / cap_q))
    assert L['eps'] <= cap and L['eps_q'] <= cap_q, (name, L['eps'], cap, L['eps_q'], cap_q)


@pytest.mark.parametrize('name', ['frames', 'irregular'])
def test_per_frame_offsets_against_float64(scene, name):
    L = scene[name]
    got = L['got']
    for what, g, w64, w32 in (('local_f', got['local_frames'], L['o64'], L['o32']), ('q_f', got['q_frames'], L['Q64'], L['Q32'])):
        a, b, c = (np.asarray(x, dtype=np.float64).reshape(x.shape[0], -1) for x in (g, w64, w32))
        scale, err, err32 = np.abs(b).max(axis=1), np.abs(a - b).max(axis=1), np.abs(c - b).max(axis=1)
        ok = scale > 0
        print('{} {}: largest row error / bar {:.3f}'.format(
            name, what, float((err[ok] / np.minimum(1e-4 * scale[ok], 4 * err32[ok] + 1e-7 * scale[ok])).max())))
        REF.check_rows('{} {}'.format(name, what), g, w64, w32)
    _check_per_frame(name, L)


# ---- 2. statistics --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['frames', 'two_groups', 'irregular'])
def test_statistics_against_float64(scene, name):
    L = scene[name]
    assert L['ref']['counts'].min() >= 2
    _check_per_frame(name, L)
    _check_statistics(name, L['got'], L['ref'], L['eps'], L['eps_q'])


# ---- 3. the shapes of the reduction ---------------------------------------------------------------------------------------
def test_group_sizes_around_the_chunk_and_degenerate_counts(scene):
    L = scene['shapes']
    counts = L['ref']['counts']
    assert [n for _, n in L['groups']] == [1, 2, 255, 0, 256, 257, 513]
    assert counts[0].tolist() == [1] * 12 and counts[1].tolist() == [2] * 12 and not counts[3].any()
    assert counts[6, 3] == 0 and counts[5, 5] == 1 and counts[6].max() > 256 * 1.8
    _check_per_frame('shapes', L)
    _check_statistics('shapes', L['got'], L['ref'], L['eps'], L['eps_q'])
    for k in STATS:
        assert np.isfinite(L['got'][k]).all(), k


# ---- 4. determinism and independence ------------------------------------------------------------------------------------
def _same_bits(a, b, what):
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def test_repeated_launches_and_groups_alone_give_the_same_bits(scene):
    L = scene['shapes']
    args = (L['faces'], L['verts'], L['ids'], L['p'], L['Rr'], L['masks'])
    first = _launch(*args, L['groups'])
    _same_bits(first, _launch(*args, L['groups']), 'second launch')
    _same_bits({k: first[k] for k in STATS}, _launch(*args, L['groups'], per_frame=False), 'without per-frame outputs')
    for g, (at, n) in enumerate(L['groups']):
        if n == 0:
            continue   # a launch needs at least one frame; the empty group is covered in the batch
        sl = slice(at, at + n)
        alone = _launch(L['faces'], L['verts'][sl], L['ids'], L['p'][sl], L['Rr'][sl], L['masks'][sl], [(0, n)])
        for k in STATS:
            assert torch.equal(alone[k][0], first[k][g]), (g, k)
        assert torch.equal(alone['local_frames'], first['local_frames'][sl])
        assert torch.equal(alone['q_frames'], first['q_frames'][sl])


def test_sub_mesh_layout_gives_the_bits_of_the_full_mesh(scene):
    """The same vertices gathered into the sensor sub-mesh, with the sensor tables in its numbering: the same kernel does
    the same arithmetic on the same values, so every output has the same bits."""
    L = scene['shapes']
    needed, sub_faces = TB.sub_mesh_vertices(L['faces'], L['ids'])
    assert len(needed) == 60
    sub_ids = np.searchsorted(needed, L['ids']).tolist()
    sub = _launch(sub_faces, np.ascontiguousarray(L['verts'][:, needed]), sub_ids, L['p'], L['Rr'], L['masks'], L['groups'])
    for k, v in sub.items():
        assert np.array_equal(v.cpu().numpy(), L['got'][k]), k


# ---- 5. end to end --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def recordings():
    """Two recordings of 1024 frames of one subject, generated as synthetic.make_windows generates its windows (5 mm
    isotropic position noise, 2 degrees of rotation noise) through the HIP get_estimated_real_markers of the small model,
    with the subject's offsets in both and make_sequence's 0.2 % of missing readings."""
    from em_pose_amd.nn.models import create_model
    model, ids = H.small_model(), REF.small_ids()
    smpl = SMPLLayer(model).to(DEV)
    net = create_model(lgd_config(12, True, 2, hidden=32, rnn_hidden=32), SMPLLayer(model))
    net.vertex_ids = ids
    net = net.to(DEV).eval()
    rng = np.random.default_rng(71)
    t = rng.normal(0.0, 0.02, (12, 3)).astype(np.float32)
    r0 = synthetic._exp_so3(rng.normal(0.0, 0.1, (12, 3))).astype(np.float32)

    def sensors(poses, betas, o_r, o_t):      # the subject's offsets, whatever the window drew
        pos, ori, _ = net.get_estimated_real_markers(gpu(poses), gpu(betas), gpu(r0[None]), gpu(t[None]),
                                                     frames_per_window=poses.shape[0])
        return pos.cpu().numpy(), ori.cpu().numpy()
    samples = []
    for seed in (72, 73):
        w = synthetic.make_windows(1, 1024, seed, sensors)
        masks = (np.random.default_rng(seed + 17).uniform(size=(1024, 12)) > 0.002).astype(np.float32)
        samples.append(RealSample('subject1_%d' % seed, w['marker_pos'][0].reshape(1024, 12, 3),
                                  w['marker_oris'][0].reshape(1024, 12, 3, 3), masks, w['poses'][0], w['shapes'][0],
                                  np.zeros((1024, 3), np.float32), {'means': None, 'covs': None, 'r': None}))
    return smpl, ids, samples, t, r0


def test_estimator_recovers_the_offsets_of_noisy_recordings(recordings, scene, tmp_path):
    smpl, ids, samples, t, r0 = recordings
    with warnings.catch_warnings():
        warnings.simplefilter('error')       # nothing to warn about: every sensor has counts and a small spread
        est = OFS.estimate_offsets(smpl, samples, subjects=['subject1', 'subject1'], vertex_ids=ids)
    assert list(est) == ['subject1']
    est = est['subject1']
    masks = np.concatenate([s.marker_masks for s in samples])
    n = masks.sum(axis=0)
    assert np.array_equal(est['counts'], n.astype(np.int32)) and n.min() > 2000 and n.min() < 2048
    assert np.array_equal(est['vertex_ids'], ids)
    d = np.abs(est['means'].astype(np.float64) - t)
    bound = 5 * 0.005 / np.sqrt(n)
    print('means: largest error / bound {:.3f}'.format(float((d / bound[:, None]).max())))
    assert (d <= bound[:, None]).all()
    cos = (np.einsum('mij,mij->m', est['r'].astype(np.float64), r0.astype(np.float64)) - 1.0) * 0.5
    angle = np.arccos(np.clip(cos, -1.0, 1.0))
    bound = 5 * np.sqrt(3.0) * np.radians(2.0) / np.sqrt(n)
    print('r: largest angle / bound {:.3f}'.format(float((angle / bound).max())))
    assert (angle <= bound).all()
    var = np.diagonal(est['covs'].astype(np.float64), axis1=-2, axis2=-1)
    rel = np.abs(var / 2.5e-5 - 1.0)
    bound = 5 * np.sqrt(2.0 / (n - 1.0))
    print('diag covs: largest relative error / bound {:.3f}'.format(float((rel / bound[:, None]).max())))
    assert (rel <= bound[:, None]).all()
    assert (est['r_spread_deg'] > 1.0).all() and (est['r_spread_deg'] < 6.0).all()     # 2 degrees per axis

    # the file goes back into the forward model: its sensors sit on the readings, up to the noise
    path = str(tmp_path / 'subject1_offsets.npz')
    OFS.save_offsets_npz(path, est)
    tr = SampleMarkersWithOffsets(smpl, [path], noise_level=-1, on_device=True)
    poses = np.stack([s.smpl_poses for s in samples])
    shapes = np.stack([s.smpl_shape for s in samples])
    batch = ABatch([0, 1], torch.full((2,), 1024, dtype=torch.long), gpu(poses), gpu(shapes),
                   torch.zeros(2, 1024, 3, device=DEV), None)
    out = tr(SMPLFK(smpl, vertex_ids=ids)(batch))
    synth = out.marker_pos_synth.cpu().numpy().astype(np.float64).reshape(2048, 12, 3)
    read = np.concatenate([s.marker_pos_real.reshape(1024, 12, 3) for s in samples]).astype(np.float64)
    resid = ((synth - read) * masks[..., None]).sum(axis=0) / n[:, None]
    bound = 5 * 0.005 / np.sqrt(n) + scene['frames']['eps']        # eps of the per-frame comparison, held to the row bar there
    print('mean residual: largest / bound {:.3f}'.format(float((np.abs(resid) / bound[:, None]).max())))
    assert (np.abs(resid) <= bound[:, None]).all()


def test_estimate_offsets_subjects_normalisation_and_warnings(recordings):
    smpl, ids, samples, _, _ = recordings
    rng = np.random.default_rng(81)
    cut = lambda s, a, b: s.extract_window(a, b)
    a, b, c = cut(samples[0], 0, 300), cut(samples[1], 100, 357), cut(samples[0], 500, 520)
    # recordings whose first root orientation is not the identity and that move: the estimator normalises a copy
    moved = []
    for s in (a, b, c):
        s = cut(s, 0, s.n_frames)
        R0 = synthetic._exp_so3(rng.normal(0, 0.7, 3))
        trans = rng.normal(0, 0.5, (s.n_frames, 3)).astype(np.float32)
        from em_pose_amd.data.transforms import matrix_to_rotvec
        from em_pose_amd.eval.metrics import rotvec_to_matrix
        poses = s.smpl_poses.copy()
        poses[:, :3] = matrix_to_rotvec(R0 @ rotvec_to_matrix(poses[:, :3].astype(np.float64))).astype(np.float32)
        pos = s.marker_pos_real.reshape(-1, 12, 3).astype(np.float64) @ R0.T + trans[:, None]
        ori = R0 @ s.marker_ori_real.reshape(-1, 12, 3, 3).astype(np.float64)
        moved.append(RealSample(s.id, pos.astype(np.float32), ori.astype(np.float32), s.marker_masks, poses,
                                s.smpl_shape, trans, {'means': None, 'covs': None, 'r': None}))
    before = [(s.marker_pos_real.copy(), s.marker_ori_real.copy(), s.smpl_poses.copy()) for s in moved]
    est = OFS.estimate_offsets(smpl, moved, subjects=['x', 'y', 'x'], vertex_ids=ids, per_frame=True)
    for s, (p0, o0, q0) in zip(moved, before):
        assert np.array_equal(s.marker_pos_real, p0) and np.array_equal(s.marker_ori_real, o0)
        assert np.array_equal(s.smpl_poses, q0)
    assert list(est) == ['x', 'y']
    assert est['x']['local_frames'].shape == (320, 12, 3) and est['y']['q_frames'].shape == (257, 12, 3, 3)
    assert int(est['x']['counts'].max()) <= 320 and int(est['y']['counts'].max()) <= 257
    # the same recordings before they were moved, pooled the same way: the frames agree to the fp32 rounding of readings
    # of about a metre that went through a rotation and a translation and back (1e-6 m), the means with them
    still = OFS.estimate_offsets(smpl, [a, b, c], subjects=['x', 'y', 'x'], vertex_ids=ids, per_frame=True)
    for k in ('x', 'y'):
        assert np.array_equal(est[k]['counts'], still[k]['counts'])
        assert np.abs(est[k]['local_frames'] - still[k]['local_frames']).max() <= 5e-6
        assert np.abs(est[k]['means'] - still[k]['means']).max() <= 5e-6
    # normalized=True takes the samples as they are: the estimate of a pre-normalised copy has the same bits
    import copy
    pre = [NormalizeRealMarkers()(copy.copy(s)) for s in moved]
    again = OFS.estimate_offsets(smpl, pre, subjects=['x', 'y', 'x'], vertex_ids=ids, normalized=True)
    for k in ('x', 'y'):
        for name in ('means', 'covs', 'r', 'counts', 'r_spread_deg'):
            assert np.array_equal(again[k][name], est[k][name]), (k, name)
    # one subject by default; a sensor that is read once, and a rotational offset that tumbles: warnings, no failure
    one = cut(samples[0], 0, 64)
    one.marker_masks = one.marker_masks.copy()
    one.marker_masks[:, 2] = 0
    one.marker_masks[5, 2] = 1
    ori = one.marker_ori_real.reshape(64, 12, 3, 3).copy()
    ori[:, 7] = ori[:, 7] @ synthetic._exp_so3(rng.normal(0, 2.0, (64, 3))).astype(np.float32)
    one.marker_ori_real = ori.reshape(64, -1)
    with pytest.warns(UserWarning) as caught:
        est = OFS.estimate_offsets(smpl, [one], vertex_ids=ids)
    text = ' | '.join(str(w.message) for w in caught)
    assert 'fewer than two valid frames' in text and 'sensors [2]' in text
    assert 'poorly determined' in text and 'sensors [7]' in text
    assert list(est) == ['all'] and est['all']['counts'][2] == 1 and not est['all']['covs'][2].any()
    assert est['all']['r_spread_deg'][7] > 45 and all(np.isfinite(v).all() for v in est['all'].values())


# ---- the script -----------------------------------------------------------------------------------------------------------
def test_script_writes_files_the_training_preprocessing_accepts(tmp_path, monkeypatch, capsys):
    """`scripts/estimate_offsets.py --synthetic --out DIR` writes one file per subject, and the files are accepted where
    `scripts/train.py --offset_files` hands them: `get_end_to_end_preprocess_fn`."""
    import importlib.util
    import os
    import sys
    from em_pose_amd.data.transforms import get_end_to_end_preprocess_fn, load_offsets_npz
    from em_pose_amd.helpers.configuration import CONSTANTS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('estimate_offsets_script', os.path.join(root, 'scripts', 'estimate_offsets.py'))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    monkeypatch.setattr(sys, 'argv', ['estimate_offsets.py', '--synthetic', '--out', str(tmp_path), '--device', DEV])
    script.main()
    printed = capsys.readouterr().out
    files = sorted(os.listdir(str(tmp_path)))
    assert files == ['synthA_offsets.npz', 'synthB_offsets.npz']
    assert 'synthA: 2 recording(s)' in printed and 'synthB: 1 recording(s)' in printed and 'spread deg' in printed
    lengths = synthetic.README_SEQUENCE_LENGTHS
    for name, frames in (('synthA', lengths[0] + lengths[1]), ('synthB', lengths[2])):
        path = str(tmp_path / (name + '_offsets.npz'))
        d = load_offsets_npz(path)
        assert d['means'].shape == (12, 3) and d['covs'].shape == (12, 3, 3) and d['r'].shape == (12, 3, 3)
        assert d['vertex_ids'].tolist() == list(CONSTANTS.VERTEX_IDS)
        z = np.load(path)
        assert (z['counts'] <= frames).all() and (z['counts'] >= 0.98 * frames).all()       # 0.2 % missing readings
        var = np.diagonal(d['covs'], axis1=-2, axis2=-1)
        assert np.abs(var / 2.5e-5 - 1.0).max() <= 5 * np.sqrt(2.0 / (z['counts'].min() - 1.0))   # the injected 5 mm
    paths = [str(tmp_path / f) for f in files]
    smpl = SMPLLayer(synthetic.make_model()).to(DEV)
    fn = get_end_to_end_preprocess_fn(lgd_config(12, True, 2, offset_noise_level=0), smpl, paths,
                                      randomize_if_configured=True, device_offsets=True, sensors_only=True)
    assert fn.sample_markers.n_offsets == 2 and fn.sample_markers.normal_dists is not None
