"""
The few transforms `evaluate_real` needs before the model sees a recording (reference empose/data/transforms.py):

  NormalizeRealMarkers   reference transforms.py:99-129  sensor readings into the frame of the first SMPL root pose
  ToTensor               reference transforms.py:51-56
  NormalizeRoot          reference transforms.py:229-256 first root orientation := identity, translation := 0
  ResampleSequence       reference scripts/preprocess_amass_3dpw.py:146-148 a sequence to 60 Hz, on the GPU

  SMPLFK, SampleMarkersWithOffsets, get_end_to_end_preprocess_fn   reference transforms.py:259-282,132-226,23-48 on the
                         HIP full-mesh kernel (pinned by tests/golden/preprocess.npz); opt-in without
                         the mesh: SMPLFK(vertex_ids=...) on the sensor sub-mesh, SampleMarkersWithOffsets(on_device=True)
                         as one launch of empose_sample_sensors_fwd (csrc/sensor_sample.hip) with a HIP reverse

The sensor-noise augmentation of the reference (noise_functions.py: spherical noise, sensor suppression) is
data/noise_functions.py on the sensor-noise kernel; `get_end_to_end_preprocess_fn` adds it with `device_noise=True` and
refuses configurations that ask for it otherwise.
"""
import numpy as np
import torch

from em_pose_amd.eval.metrics import rotvec_to_matrix


def matrix_to_rotvec(R):
    """(...,3,3) -> (...,3) log map, float64, robust near 0 and pi."""
    R = np.asarray(R, dtype=np.float64)
    tr = np.clip((np.trace(R, axis1=-2, axis2=-1) - 1.0) * 0.5, -1.0, 1.0)
    theta = np.arccos(tr)
    w = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    s = np.sin(theta)
    small = theta < 1e-6
    near_pi = (np.pi - theta) < 1e-4
    scale = np.where(small, 0.5 + theta ** 2 / 12.0, theta / (2.0 * np.where(np.abs(s) < 1e-12, 1.0, s)))
    out = w * scale[..., None]
    if np.any(near_pi):
        # axis from the symmetric part: R + I = 2 n n^T at theta = pi
        B = (R + np.eye(3)) * 0.5
        k = np.argmax(np.diagonal(B, axis1=-2, axis2=-1), axis=-1)
        col = np.take_along_axis(B, k[..., None, None], axis=-1)[..., 0]
        axis = col / np.linalg.norm(col, axis=-1, keepdims=True)
        axis = axis * np.where((axis * w).sum(-1, keepdims=True) < 0, -1.0, 1.0)
        out = np.where(near_pi[..., None], axis * theta[..., None], out)
    return out


class NormalizeRealMarkers(object):
    def __call__(self, sample):
        n_markers = sample.marker_pos_real.shape[-1] // 3
        R0 = rotvec_to_matrix(np.asarray(sample.smpl_poses[0, :3], dtype=np.float64))  # (3,3)
        # the translation is removed in the dtype of the recording (reference transforms.py:109), the rotation in float64
        pos = np.asarray(sample.marker_pos_real).reshape(-1, n_markers, 3) - np.asarray(sample.smpl_trans)[:, None, :]
        pos = pos.astype(np.float64) @ R0  # R0^T p for row vectors
        ori = R0.T @ np.asarray(sample.marker_ori_real, dtype=np.float64).reshape(-1, n_markers, 3, 3)
        sample.marker_pos_real = pos.reshape(-1, n_markers * 3).astype(np.float32)
        sample.marker_ori_real = ori.reshape(-1, n_markers * 9).astype(np.float32)
        return sample


class ToTensor(object):
    def __call__(self, sample):
        sample.to_tensor()
        return sample


class IdentityTransform(object):
    def __call__(self, sample):
        return sample


class ExtractWindow(object):
    """A window of `window_size` frames from a sample (reference transforms.py:66-96): at the beginning, around the
    middle, or at a position drawn from `rng` (a numpy RandomState); shorter samples are returned whole, unpadded."""

    def __init__(self, window_size, rng=None, mode='random'):
        if mode not in ('random', 'beginning', 'middle'):
            raise ValueError("Mode '{}' for window extraction unknown.".format(mode))
        if mode == 'random' and rng is None:
            raise ValueError('random window extraction needs an rng')
        self.window_size, self.rng, self.mode = window_size, rng, mode

    def __call__(self, sample):
        n, ws = sample.n_frames, self.window_size
        if n <= ws:
            return sample
        if self.mode == 'beginning':
            sf = 0
        elif self.mode == 'middle':
            sf = n // 2 - ws // 2
        else:
            sf = self.rng.randint(0, n - ws + 1)
        return sample.extract_window(sf, sf + ws)


class ResampleSequence(object):
    """An `AMASSSample` resampled to `fps` by the resampling kernels (data/resample.py): poses[:, :66] as 22 rotations by
    SQUAD, trans by the not-a-knot cubic spline, `fps` set to the target (`n_frames` follows the arrays).  `joints`, when
    the sample has them, are recomputed from the resampled poses through `smpl_model.fk_joints`, which must then be
    given.  A sample already at `fps` is returned untouched.  Needs a GPU: there is no host path."""

    def __init__(self, fps=None, smpl_model=None, device=None):
        from em_pose_amd.helpers.configuration import CONSTANTS as C
        self.fps = float(C.FPS if fps is None else fps)
        self.smpl_model, self.device = smpl_model, device

    def __call__(self, sample):
        from em_pose_amd.data.resample import resample_samples
        return resample_samples([sample], self.fps, self.smpl_model, self.device)[0]


class NormalizeRoot(object):
    """`on_device=True` (CUDA batches only): the root orientations are normalised by one launch of the root-frame kernel
    (empose_root_frame_fwd over N * F frames in segments of F) instead of the float64 host round trip: no `.cpu()`, no
    synchronisation.  The default is the host path."""

    def __init__(self, normalize_root_ori=True, remove_root_trans=True, on_device=False, rodrigues_convention='smplx'):
        self.normalize_root_ori = normalize_root_ori
        self.remove_root_trans = remove_root_trans
        self.on_device = on_device
        self.rodrigues_convention = rodrigues_convention

    def __call__(self, batch):
        with torch.no_grad():
            batch.trans_source = batch.trans.clone()
            batch.root_pose_source = batch.poses[:, :, :3].clone()
            if self.remove_root_trans:
                batch.trans = torch.zeros_like(batch.trans)
            if self.normalize_root_ori and self.on_device:
                from em_pose_amd import _lib
                from em_pose_amd.bodymodels.smpl import root_frame_fwd
                n, f, ld = batch.poses.shape
                rows = batch.poses.detach().reshape(n * f, ld).contiguous().float()
                root, _ = root_frame_fwd(rows, None, f, _lib.RODRIGUES[self.rodrigues_convention])
                batch.poses = batch.poses.clone()
                batch.poses[:, :, :3] = root.reshape(n, f, 3).to(batch.poses.dtype)
            elif self.normalize_root_ori:
                root = batch.poses[:, :, :3].detach().cpu().numpy().astype(np.float64)
                R = rotvec_to_matrix(root)  # (N,F,3,3)
                Rn = np.swapaxes(R[:, :1], -1, -2) @ R
                batch.poses = batch.poses.clone()
                batch.poses[:, :, :3] = torch.from_numpy(matrix_to_rotvec(Rn)).to(batch.poses)
        return batch


class SMPLFK(object):
    """Ground-truth joints and vertices for a batch (reference transforms.py:259-282) through the HIP full-mesh layer.
    With `vertex_ids` (the sensor vertices) only the sensor sub-mesh is evaluated (`smpl_model.sub_mesh(vertex_ids)`):
    `batch.vertices` is (n, f, len(needed) * 3) and `batch.vertices_subset` holds `needed`, the original ids of its
    vertices; the joints are the same.  `SampleMarkersWithOffsets` reads either."""

    def __init__(self, smpl_model, vertex_ids=None):
        self.smpl_model = smpl_model
        self.vertex_ids = None if vertex_ids is None else tuple(int(v) for v in vertex_ids)
        self.max_window_size = 1000

    def __call__(self, batch):
        n, f = batch.batch_size, batch.seq_length
        p = batch.poses_body.reshape(n * f, -1)
        s = batch.shapes.unsqueeze(1).repeat(1, f, 1).reshape(n * f, -1)
        r = batch.poses_root.reshape(n * f, -1)
        t = batch.trans.reshape(n * f, -1)
        layer = self.smpl_model if self.vertex_ids is None else self.smpl_model.sub_mesh(self.vertex_ids)
        vertices, joints = layer(poses_body=p, betas=s, poses_root=r, trans=t, window_size=self.max_window_size)
        batch.joints_gt = joints[:, :22].reshape(n, f, -1)
        batch.vertices = vertices.reshape(n, f, -1)
        batch.vertices_subset = None if self.vertex_ids is None else layer.needed
        batch.joints_hat = batch.joints_gt.clone().detach()
        return batch


def load_offsets_npz(path):
    """One `*_offsets.npz` file of the reference (transforms.py:145-155): per-sensor offset means (M,3), covariances
    (M,3,3), local-to-global orientation offsets r (M,3,3) and the sensor vertex ids (M,)."""
    d = np.load(path)
    return {'means': d['means'], 'covs': d['covs'] if 'covs' in d.files else None, 'r': d['r'],
            'vertex_ids': d['vertex_ids']}


class SampleMarkersWithOffsets(object):
    """
    Virtual sensors sampled from the ground-truth mesh with per-subject offsets applied (reference
    transforms.py:132-226).  `offset_sets` is a list of dicts with `means` (M,3), `covs` (M,3,3), `r` (M,3,3) and
    `vertex_ids` (M,) -- the content of the reference's `*_offsets.npz` files, or the paths of such files; one set is
    drawn per batch entry with the reference's seeded RandomState(6273).

    `noise_level` as in the reference: -1 deterministic (offsets = the stored means; evaluation), 0 one offset draw per
    window from N(means, covs), 1 one draw per frame, 2 no positional offset, 3 no positional and no rotational offset.
    The draws come from torch's global generator (`MultivariateNormal.sample`), like the reference's.
    `offset_t_augmented` always carries the means: that is what is known at test time.

    `on_device=True`: frames and offsets are one launch (empose_sample_sensors_fwd, csrc/sensor_sample.hip) instead of
    the sensor kernel followed by a dozen small torch launches.  The host draws are the same calls in the same order
    (`plan`); the gathered means, the gathered r and the selected draws go up in one pinned block with one copy that
    does not block, and nothing in `__call__` waits for the device.  When `batch.vertices` requires grad the call is an
    autograd node whose backward is empose_sample_sensors_vjp (single backward only; no gradient for the offsets).

    Either path accepts a sub-mesh batch (`batch.vertices_subset`, SMPLFK(vertex_ids=...)): the sensors are then read
    with the topology restricted to the subset, in its numbering.  A subset without a sensor's fan raises ValueError.
    """

    def __init__(self, smpl_model, offset_sets, noise_level=-1, on_device=False):
        from em_pose_amd.data.virtual_sensors import VirtualMarkerHelper
        if isinstance(offset_sets, (dict, str)):
            offset_sets = [offset_sets]
        # the reference passes `*_offsets.npz` paths (transforms.py:142-155: keys means, covs, r, vertex_ids)
        offset_sets = [load_offsets_npz(o) if isinstance(o, str) else o for o in offset_sets]
        if noise_level not in (-1, 0, 1, 2, 3):
            raise ValueError('Unknown noise level {}'.format(noise_level))
        self.noise_level = noise_level
        self.randomize = noise_level >= 0
        self.n_offsets = len(offset_sets)
        self.offset_means = np.stack([np.asarray(o['means'], dtype=np.float32) for o in offset_sets])
        self.r = np.stack([np.asarray(o['r'], dtype=np.float32) for o in offset_sets])
        self.vertex_ids = [int(v) for v in np.asarray(offset_sets[-1]['vertex_ids']).tolist()]
        self.smpl_model, self.on_device = smpl_model, on_device
        self.virtual_helper = VirtualMarkerHelper(smpl_model)
        self._subset_helpers = {}
        self.offset_rng = np.random.RandomState(6273)
        self.normal_dists = None
        if noise_level in (0, 1):
            if any(o.get('covs') is None for o in offset_sets):
                raise ValueError('noise levels 0 and 1 need the offset covariances (`covs`)')
            covs = np.stack([np.asarray(o['covs'], dtype=np.float32) for o in offset_sets])
            self.normal_dists = torch.distributions.MultivariateNormal(
                loc=torch.from_numpy(self.offset_means), covariance_matrix=torch.from_numpy(covs))

    def _helper_and_ids(self, batch):
        """The helper and the sensor ids in the numbering of `batch.vertices`: the body model's, or for a sub-mesh
        batch those of the sensor topology restricted to `batch.vertices_subset` (ascending original ids)."""
        subset = getattr(batch, 'vertices_subset', None)
        if subset is None:
            return self.virtual_helper, self.vertex_ids
        from em_pose_amd.bodymodels import tables as TB
        from em_pose_amd.data.virtual_sensors import VirtualMarkerHelper
        subset = np.asarray(subset.detach().cpu() if torch.is_tensor(subset) else subset, dtype=np.int64).reshape(-1)
        key = (subset.tobytes(), getattr(self.smpl_model, 'tables_version', 0))
        if key not in self._subset_helpers:
            if np.any(np.diff(subset) <= 0):
                raise ValueError('vertices_subset must hold ascending vertex ids')
            needed, faces = TB.sub_mesh_vertices(self.smpl_model.model['f'], self.vertex_ids)
            if not np.isin(needed, subset).all():
                raise ValueError('vertices_subset lacks vertices {} of the sensors\' fans'.format(
                    needed[~np.isin(needed, subset)].tolist()))
            stub = type('SubMeshFaces', (object,), {})()
            stub.model = {'f': np.searchsorted(subset, needed[faces])}   # the restricted faces, renumbered by position
            ids = [int(i) for i in np.searchsorted(subset, np.asarray(self.vertex_ids, dtype=np.int64))]
            self._subset_helpers = {key: (VirtualMarkerHelper(stub), ids)}   # one subset at a time
        return self._subset_helpers[key]

    def plan(self, n, f):
        """The host side of one call, the reference's draws in its order -- the offset sets from RandomState(6273), then
        `MultivariateNormal.sample` from torch's global generator with the shapes of the torch path -- as
        (means (n, M, 3), r (n, M, 3, 3) with the identity at level 3, local, mode): `local` is (n, M, 3) for
        SAMPLE_LOCAL_WINDOW, (n, f, M, 3) for SAMPLE_LOCAL_FRAME, None for SAMPLE_LOCAL_NONE.  Host float32 tensors."""
        from em_pose_amd import _lib
        s_np = self.offset_rng.randint(0, self.n_offsets, n)
        s_idxs = torch.from_numpy(s_np).long()
        means = torch.from_numpy(self.offset_means[s_np])
        r = torch.from_numpy(self.r[s_np])
        local, mode = means, _lib.SAMPLE_LOCAL_WINDOW
        if self.noise_level == 0:
            local = self.normal_dists.sample((n,))[torch.arange(n), s_idxs]
        elif self.noise_level == 1:
            local, mode = self.normal_dists.sample((n, f))[torch.arange(n), :, s_idxs], _lib.SAMPLE_LOCAL_FRAME
        elif self.noise_level in (2, 3):
            local, mode = None, _lib.SAMPLE_LOCAL_NONE
        if self.noise_level == 3:
            r = torch.eye(3).expand(n, r.shape[1], 3, 3).contiguous()
        return means, r, local, mode

    def _call_on_device(self, batch):
        from em_pose_amd.data.noise_functions import _Plan
        n, f = batch.batch_size, batch.seq_length
        helper, ids = self._helper_and_ids(batch)
        vs = batch.vertices.reshape(n * f, -1, 3)
        if not vs.is_cuda:
            from em_pose_amd import _lib
            raise _lib.EmposeError('SampleMarkersWithOffsets(on_device=True) needs GPU tensors; there is no CPU fallback')
        means, r, local, mode = self.plan(n, f)
        arrays = {'means': means, 'r': r}
        if local is not None and self.noise_level >= 0:
            arrays['local'] = local.float()
        with torch.cuda.device(vs.device):
            dev = _Plan(arrays).upload(vs.device)
        local_dev = dev.get('local', dev['means']) if local is not None else None
        r_dev = None if self.noise_level == 3 else dev['r']    # the kernel's identity: no product
        if torch.is_grad_enabled() and vs.requires_grad:
            outs = _SampleSensorsFn.apply(helper, vs, tuple(ids), f, mode, local_dev, r_dev)
        else:
            outs = sample_sensors_fwd(helper, vs.contiguous().float(), ids, f, mode, local_dev, r_dev)
        m = len(ids)
        for name, x in zip(('marker_pos_vertex', 'marker_ori_vertex', 'marker_normal_vertex', 'marker_pos_synth',
                            'marker_ori_synth', 'marker_normal_synth'), outs):
            setattr(batch, name, x.reshape(n, f, -1))
        batch.offset_t_augmented = dev['means']
        batch.offset_r_augmented = dev['r']
        return batch

    def __call__(self, batch):
        if self.on_device:
            return self._call_on_device(batch)
        n, f = batch.batch_size, batch.seq_length
        vs = batch.vertices.reshape(n * f, -1, 3)
        helper, ids = self._helper_and_ids(batch)
        markers, oris, normals = helper.get_virtual_pos_and_rot(vs, ids)
        dev = markers.device
        batch.marker_pos_vertex = markers.reshape(n, f, -1)
        batch.marker_ori_vertex = oris.reshape(n, f, -1)
        batch.marker_normal_vertex = normals.reshape(n, f, -1)
        s_np = self.offset_rng.randint(0, self.n_offsets, n)
        s_idxs = torch.from_numpy(s_np).long()
        means = torch.from_numpy(self.offset_means[s_np]).to(dev)  # (n, M, 3)
        r = torch.from_numpy(self.r[s_np]).to(dev)  # (n, M, 3, 3)
        local = means[:, None].expand(n, f, means.shape[1], 3)
        if self.noise_level == 0:      # one draw per window
            draw = self.normal_dists.sample((n,))[torch.arange(n), s_idxs]  # (n, M, 3)
            local = draw.to(dev)[:, None].expand(n, f, draw.shape[1], 3)
        elif self.noise_level == 1:    # one draw per frame
            draw = self.normal_dists.sample((n, f))  # (n, f, n_offsets, M, 3)
            local = draw[torch.arange(n), :, s_idxs].to(dev)  # (n, f, M, 3)
        elif self.noise_level in (2, 3):
            local = torch.zeros(n, f, means.shape[1], 3, device=dev)
        if self.noise_level == 3:
            r = torch.eye(3, device=dev).expand(n, r.shape[1], 3, 3).contiguous()
        ori = oris.reshape(n, f, -1, 3, 3)
        pos = markers.reshape(n, f, -1, 3) + torch.matmul(ori, local.to(ori.dtype).unsqueeze(-1)).squeeze(-1)
        ori = torch.matmul(ori, r[:, None])
        batch.marker_pos_synth = pos.reshape(n, f, -1)
        batch.marker_ori_synth = ori.reshape(n, f, -1)
        batch.marker_normal_synth = ori[..., 2].reshape(n, f, -1)
        batch.offset_t_augmented = means
        batch.offset_r_augmented = r
        return batch


def sample_sensors_fwd(helper, v, vertex_ids, f, mode, local, r):
    """empose_sample_sensors_fwd on fp32 contiguous vertices (n * f, V, 3) with `helper`'s tables (VirtualMarkerHelper):
    (pos, ori, normals, pos_synth, ori_synth, normal_synth).  `local`, `r`: device tensors by `mode`, or None."""
    from em_pose_amd import _lib
    t, nv, m = v.shape[0], v.shape[1], len(vertex_ids)
    center, hlp, deg, faces, max_deg = helper._tables(vertex_ids, v.device)
    new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=v.device)
    with torch.cuda.device(v.device):
        outs = (new(t, m, 3), new(t, m, 3, 3), new(t, m, 3), new(t, m, 3), new(t, m, 3, 3), new(t, m, 3))
        _lib.check(_lib.lib().empose_sample_sensors_fwd(
            t // f, f, nv, _lib.dptr(v), m, max_deg, _lib.dptr(center), _lib.dptr(hlp), _lib.dptr(deg), _lib.dptr(faces),
            mode, _lib.dptr(local), _lib.dptr(r), *[_lib.dptr(o) for o in outs], _lib.current_stream()))
    return outs


def sample_sensors_vjp(helper, v, vertex_ids, f, mode, local, r, cotangents):
    """empose_sample_sensors_vjp: d_vertices (n * f, V, 3) fp32 for the six cotangents (any but not all may be None)."""
    from em_pose_amd import _lib
    t, nv, m = v.shape[0], v.shape[1], len(vertex_ids)
    center, hlp, deg, faces, max_deg = helper._tables(vertex_ids, v.device)
    rev = helper._reverse_tables(vertex_ids, nv, v.device)
    lib = _lib.lib()
    with torch.cuda.device(v.device):
        d_v = torch.empty(t, nv, 3, dtype=torch.float32, device=v.device)
        ws_bytes = lib.empose_sample_sensors_vjp_workspace_bytes(t, m)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=v.device)
        _lib.check(lib.empose_sample_sensors_vjp(
            t // f, f, nv, _lib.dptr(v), m, max_deg, _lib.dptr(center), _lib.dptr(hlp), _lib.dptr(deg), _lib.dptr(faces),
            rev[0].shape[0], *[_lib.dptr(a) for a in rev[:7]], rev[7].shape[0], _lib.dptr(rev[7]),
            mode, _lib.dptr(local), _lib.dptr(r), *[_lib.dptr(c) for c in cotangents],
            _lib.dptr(d_v), _lib.dptr(ws), ws_bytes, _lib.current_stream()))
    return d_v


class _SampleSensorsFn(torch.autograd.Function):
    """`SampleMarkersWithOffsets(on_device=True)` under autograd: the forward is the launch of the no-grad call; the
    backward is empose_sample_sensors_vjp on the saved vertices (single backward only).  `local` and `r` are
    constants."""

    @staticmethod
    def forward(ctx, helper, vertices, vertex_ids, f, mode, local, r):
        ctx.helper, ctx.vertex_ids, ctx.f, ctx.mode = helper, vertex_ids, f, mode
        ctx.save_for_backward(vertices, local, r)
        ctx.set_materialize_grads(False)
        return sample_sensors_fwd(helper, vertices.contiguous().float(), vertex_ids, f, mode, local, r)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *cotangents):
        if all(c is None for c in cotangents):
            return (None,) * 7
        vertices, local, r = ctx.saved_tensors
        f32 = lambda t: t.contiguous().float() if t is not None else None
        d_v = sample_sensors_vjp(ctx.helper, f32(vertices), ctx.vertex_ids, ctx.f, ctx.mode, local, r,
                                 [f32(c) for c in cotangents])
        return (None, d_v.to(vertices.dtype).reshape(vertices.shape)) + (None,) * 5


def get_end_to_end_preprocess_fn(config, smpl_model, offset_files, randomize_if_configured=False,
                                 device_normalize=False, device_noise=False, device_offsets=False, sensors_only=False):
    """
    The reference's preprocessing factory (transforms.py:23-48): NormalizeRoot -> SMPLFK -> SampleMarkersWithOffsets ->
    sensor noise, with the configured offset noise level when `randomize_if_configured`.  `offset_files`: the
    `*_offsets.npz` files (the reference takes them from its data directory).  `device_normalize`:
    NormalizeRoot(on_device=True).  `device_noise`: the reference's sensor-noise function (`get_noise_fn`) on the
    sensor-noise kernel (data/noise_functions.py; GPU batches only); it runs after the sensors are sampled and receives
    the keyword arguments of the call, as in the reference.  Without the switch a configuration that asks for sensor noise
    is refused.  `device_offsets`: SampleMarkersWithOffsets(on_device=True), the sensors and their offsets in one launch.
    `sensors_only`: SMPLFK evaluates the sensor sub-mesh only (SMPLFK(vertex_ids=the sensors')), so `batch.vertices` holds
    the vertices the sensors read instead of the mesh.  All four switches compose; all are off by default.
    """
    if not getattr(config, 'use_real_offsets', True):
        raise ValueError('We expect to use the real offsets.')
    noise_fn = None
    if device_noise:
        from em_pose_amd.data.noise_functions import get_noise_fn, no_noise
        noise_fn = get_noise_fn(config, randomize_if_configured)
        noise_fn = None if noise_fn is no_noise else noise_fn
    elif randomize_if_configured and (getattr(config, 'spherical_noise_length', 0.0) > 0.0 or
                                      getattr(config, 'suppression_noise_length', 0.0) > 0.0):
        # The reference would now add its sensor-noise augmentation (noise_functions.py:14-36: spherical marker noise or
        # marker suppression).  It runs on the GPU only and is opt-in: refuse instead of silently training without it.
        raise NotImplementedError('sensor-noise augmentation (spherical_noise_length / suppression_noise_length > 0) '
                                  'is not implemented in this build without device_noise=True (the sensor-noise kernel)')
    noise_level = getattr(config, 'offset_noise_level', -1) if randomize_if_configured else -1
    sample_markers = SampleMarkersWithOffsets(smpl_model, list(offset_files), noise_level=noise_level,
                                              on_device=device_offsets)
    normalize_root = NormalizeRoot(on_device=device_normalize)
    fk = SMPLFK(smpl_model, vertex_ids=sample_markers.vertex_ids if sensors_only else None)

    def _preprocess_fn(sample, mode='all', **noise_kwargs):
        noise = (lambda b: noise_fn(b, **noise_kwargs)) if noise_fn is not None else (lambda b: b)
        if mode == 'all':
            return noise(sample_markers(fk(normalize_root(sample))))
        if mode == 'normalize_only':
            return normalize_root(sample)
        if mode == 'after_normalize':
            return noise(sample_markers(fk(sample)))
        raise ValueError("Mode '{}' unknown.".format(mode))
    _preprocess_fn.noise_fn = noise_fn   # None: the plain pipeline
    _preprocess_fn.fk, _preprocess_fn.sample_markers = fk, sample_markers
    return _preprocess_fn
