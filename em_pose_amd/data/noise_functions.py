"""
Sensor-noise augmentation of the training data path (reference empose/data/noise_functions.py): `get_noise_fn`,
`SphericalMarkerNoise`, `MarkerSuppressionNoise`, with the reference's names, constructor signatures, seeds and order of
draws.

The draws are a few hundred numbers and stay on the host, in the reference's seeded generators, so a configuration
draws here what it draws there (on the same torch build).  What the reference then does in a Python loop over the batch
entries with three indexed writes each is one launch here (`empose_sensor_noise`, csrc/sensor_noise.hip): the plan --
first frames, sensor ids, draws -- goes up from pinned memory in one copy that does not block, and nothing in `__call__`
waits for the device.  Batches live on the GPU; a CPU batch raises `_lib.EmposeError`, there is no fallback.
"""
import numpy as np
import torch

from em_pose_amd import _lib
from em_pose_amd.helpers.configuration import CONSTANTS as C

SPHERICAL, SUPPRESS = 0, 1   # EMPOSE_SENSOR_NOISE_* (include/empose_hip.h)


SEEDS = {'spherical': 98052, 'suppression': 8004}            # the reference's generator seeds
SENSOR_IDS = {12: tuple(range(12)), 6: tuple(C.S_CONFIG_6)}  # the batch's sensors a model with n inputs reads


def _unit(x):
    """`x` clamped to [0, 1]."""
    return min(1.0, max(0.0, x))


def no_noise(x, **kwargs):
    return x


def get_noise_fn(config, randomize_if_configured, is_valid=False):
    """What the configuration asks for, as a callable on batches.  Training (`randomize_if_configured`): spherical noise
    when its length is above 0, else suppression when its length is above 0 -- both at once is an error, as in the
    reference.  Otherwise only validation (`is_valid`) gets noise, and only suppression.  Everything else: `no_noise`."""
    spherical, suppression = config.spherical_noise_length > 0.0, config.suppression_noise_length > 0.0
    if randomize_if_configured and spherical:
        if suppression:
            raise AssertionError('spherical and suppression noise are both configured: only one noise type at a time')
        return SphericalMarkerNoise(config.spherical_noise_strength, config.spherical_noise_length,
                                    config.noise_num_markers)
    if suppression and (randomize_if_configured or is_valid):
        return MarkerSuppressionNoise(config.suppression_noise_length, config.noise_num_markers,
                                      config.suppression_noise_value, config.n_markers)
    return no_noise


class _Plan(object):
    """The integers and floats of one call in ONE block of host memory (pinned when there is a GPU), every array on a
    256-byte boundary: `host[name]` are views of the block, `upload` gives the same views of its one device copy."""

    def __init__(self, arrays):
        self.layout, at = {}, 0
        for name, t in arrays.items():
            assert t.dtype in (torch.int32, torch.float32)
            self.layout[name] = (at, t.dtype, tuple(t.shape))
            at += (t.numel() + 63) // 64 * 64
        self.block = torch.empty(max(at, 64), dtype=torch.int32, pin_memory=torch.cuda.is_available())
        self.host = self._views(self.block)
        for name, t in arrays.items():
            self.host[name].copy_(t)

    def _views(self, block):
        out = {}
        for name, (at, dtype, shape) in self.layout.items():
            out[name] = block[at:at + int(np.prod(shape, dtype=np.int64))].view(dtype).view(shape)
        return out

    def upload(self, device):
        return self._views(self.block.to(device, non_blocking=True))


def _host_ptr(t):
    return _lib.C.c_void_p(t.data_ptr())


def _sensor_rows(x, what):
    """(N, F, M * c) float32 readings on the GPU, contiguous."""
    if not torch.is_tensor(x) or not x.is_cuda:
        raise _lib.EmposeError('sensor noise needs the HIP path: {} must be a tensor on the GPU; there is no CPU fallback'
                               .format(what))
    if x.dtype != torch.float32:
        raise _lib.EmposeError('{} must be float32'.format(what))
    return x.detach().contiguous()


class SphericalMarkerNoise(object):
    """Displaces `num_markers` sensors (the same ones for the whole batch) inside a sphere, frame by frame, over one random
    window per batch entry.  `sphere_size` is the sphere's diameter as a share of the thigh length, `window_size` the
    window's length as a share of the sequence; both are clamped to [0, 1].  Writes `marker_pos_noisy` only."""

    def __init__(self, sphere_size, window_size, num_markers):
        self.max_r, self.ws, self.num_markers = _unit(sphere_size), _unit(window_size), num_markers
        if self.ws == 0.0 and self.max_r > 0.0:
            raise ValueError("Temporal length of spherical marker noise is 0.0 but strength is > 0.0.")
        self.rng = torch.Generator().manual_seed(SEEDS['spherical'])

    def plan(self, batch_size, seq_len, n_markers):
        """The draws of one call, in the reference's order: the sensors (shared by the batch), the first frames, the radii
        (from torch's GLOBAL generator: the reference passes none there), then the two angles."""
        m_ids = torch.randperm(n_markers, generator=self.rng)[:self.num_markers]
        window_len = int(self.ws * seq_len)
        sf = torch.randint(0, seq_len - window_len + 1, (batch_size,), generator=self.rng)
        shape = (batch_size, window_len, self.num_markers)
        u_r = torch.rand(*shape)
        thetas = torch.rand(shape, generator=self.rng) * np.pi * 2
        phis = torch.rand(shape, generator=self.rng) * np.pi
        return window_len, _Plan({'start': sf.to(torch.int32), 'sensor': m_ids.to(torch.int32), 'u_r': u_r,
                                  'theta': thetas, 'phi': phis})

    def __call__(self, batch, **kwargs):
        if self.max_r == 0.0 or batch.marker_pos_synth is None:   # nothing to displace: the batch as it is, no draws
            return batch
        pos = _sensor_rows(batch.marker_pos_synth, 'marker_pos_synth')
        n, f, m = pos.shape[0], pos.shape[1], pos.shape[-1] // 3
        window_len, plan = self.plan(n, f, m)
        with torch.cuda.device(pos.device):
            dev = plan.upload(pos.device)
            out = torch.empty_like(pos)
            _lib.check(_lib.lib().empose_sensor_noise(
                SPHERICAL, n, f, m, self.num_markers, window_len, _host_ptr(plan.host['start']),
                _host_ptr(plan.host['sensor']), _lib.dptr(dev['start']), _lib.dptr(dev['sensor']), _lib.dptr(dev['u_r']),
                _lib.dptr(dev['theta']), _lib.dptr(dev['phi']), self.max_r, C.THIGH_UPPER_IDX, C.THIGH_LOWER_IDX, 0.0,
                _lib.dptr(pos), None, None, _lib.dptr(out), None, None, _lib.current_stream()))
        batch.marker_pos_noisy = out.reshape(n, f, -1)
        return batch


class MarkerSuppressionNoise(object):
    """Makes `num_markers` sensors per batch entry (drawn with replacement from the sensors a model with `n_markers_in`
    inputs reads) read `mask_value` in position, orientation and normal over one random window per entry; `window_size`
    is the window's length as a share of the sequence, clamped to [0, 1].  Writes all three `marker_*_noisy` fields."""

    def __init__(self, window_size, num_markers, mask_value, n_markers_in=12):
        if n_markers_in not in SENSOR_IDS:
            raise AssertionError('n_markers_in must be one of {}'.format(sorted(SENSOR_IDS)))
        self.ws, self.num_markers, self.mask_value = _unit(window_size), num_markers, mask_value
        self.marker_ids = torch.tensor(SENSOR_IDS[n_markers_in], dtype=torch.long)
        self.rng = torch.Generator()
        self.reset_rng()

    def reset_rng(self):
        """The generator back at its seed: the next call draws what the first call drew."""
        self.rng.manual_seed(SEEDS['suppression'])

    def plan(self, batch_size, seq_len):
        """The draws of one call, in the reference's order: the sensors of every batch entry, then the first frames."""
        m_ids = torch.randint(0, len(self.marker_ids), (batch_size, self.num_markers), generator=self.rng)
        window_len = int(self.ws * seq_len)
        sf = torch.randint(0, seq_len - window_len + 1, (batch_size,), generator=self.rng)
        return window_len, _Plan({'start': sf.to(torch.int32), 'sensor': self.marker_ids[m_ids].to(torch.int32)})

    def __call__(self, batch, **kwargs):
        if kwargs.get('reset_rng'):
            self.reset_rng()
        pos = _sensor_rows(batch.marker_pos_synth, 'marker_pos_synth')
        ori = _sensor_rows(batch.marker_ori_synth, 'marker_ori_synth')
        normal = _sensor_rows(batch.marker_normal_synth, 'marker_normal_synth')
        n, f, m = pos.shape[0], pos.shape[1], pos.shape[-1] // 3
        if tuple(ori.shape) != (n, f, m * 9) or tuple(normal.shape) != (n, f, m * 3):
            raise _lib.EmposeError('marker_ori_synth / marker_normal_synth do not have the sensors of marker_pos_synth')
        window_len, plan = self.plan(n, f)
        with torch.cuda.device(pos.device):
            dev = plan.upload(pos.device)
            outs = [torch.empty_like(x) for x in (pos, ori, normal)]
            _lib.check(_lib.lib().empose_sensor_noise(
                SUPPRESS, n, f, m, self.num_markers, window_len, _host_ptr(plan.host['start']),
                _host_ptr(plan.host['sensor']), _lib.dptr(dev['start']), _lib.dptr(dev['sensor']), None, None, None, 0.0,
                0, 0, float(self.mask_value), _lib.dptr(pos), _lib.dptr(ori), _lib.dptr(normal), _lib.dptr(outs[0]),
                _lib.dptr(outs[1]), _lib.dptr(outs[2]), _lib.current_stream()))
        batch.marker_pos_noisy, batch.marker_ori_noisy, batch.marker_normal_noisy = outs
        return batch
