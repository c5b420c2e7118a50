"""
Model-free sensor fitting: a pose per frame and a shape per window from sensor readings alone, by K steps of Adam on the
in-loop reconstruction energy plus priors -- `empose_sensor_fit` (csrc/api_fit.hip, csrc/sensor_fit.hip; the objective is
written out in DESIGN.md section 9 and include/empose_hip.h).  No trained weights are involved: the fitter is the
hand-written first-order baseline the learned loop is motivated against (reference models.py:547-600 is this loop with the
step learned), and a polish stage after it (`init=` a model's output).
"""
import ctypes as C

import torch

from em_pose_amd import _lib
from em_pose_amd.helpers.configuration import lgd_config
from em_pose_amd.nn.models import IterativeErrorFeedback, _cat_windows, pack_sensor_inputs


class SensorFitter(object):
    """
    Wraps an `IterativeErrorFeedback` for its SMPL tables, `vertex_ids`, `marker_idxs` and input packing only: the
    weights are never read and the body-model-only handle is what the fit runs on.
    """

    def __init__(self, net, num_steps=30, lr=0.05, lr_decay=1.0, beta1=0.9, beta2=0.999, eps=1e-8, lambda_pose=1e-3,
                 lambda_shape=1e-3, lambda_smooth=1.0, shape_per_window=True, keep_best=True):
        if not isinstance(net, IterativeErrorFeedback):
            raise TypeError('SensorFitter wraps an IterativeErrorFeedback (see SensorFitter.from_smpl)')
        self.net = net
        self.num_steps = int(num_steps)
        self.lr, self.lr_decay, self.beta1, self.beta2, self.eps = lr, lr_decay, beta1, beta2, eps
        self.lambda_pose, self.lambda_shape, self.lambda_smooth = lambda_pose, lambda_shape, lambda_smooth
        self.shape_per_window, self.keep_best = bool(shape_per_window), bool(keep_best)
        self._workspace = None

    @classmethod
    def from_smpl(cls, smpl_model, n_markers=12, vertex_ids=None, **kwargs):
        """The smallest net that carries the body model and the sensor subset (its networks are never evaluated)."""
        net = IterativeErrorFeedback(lgd_config(n_markers, False, 1, hidden=8), smpl_model)
        if vertex_ids is not None:
            net.vertex_ids = [int(v) for v in vertex_ids]
        return cls(net, **kwargs)

    def fit_tensors(self, marker_pos, marker_oris, offset_t, offset_r, marker_masks=None, seq_lengths=None, init=None,
                    prior=None):
        """
        One window batch through `empose_sensor_fit`.  All tensors on the GPU: marker_pos (B,F,36), marker_oris (B,F,108),
        offsets per window, marker_masks (B,F,12) or None, seq_lengths (B,) or None; init: (pose (B,F,66), shape
        (B,F,10)) or None (zeros); prior: pose (B,F,66) or None (zeros).
        :return: dict(pose (B,F,66), shape (B,F,10), joints (B,F,66), pos (B,F,36), ori (B,F,108),
                      objective (K + 2, B): J of the iterates 0 .. K, then of what is returned; energy (B,F))
        """
        if not marker_pos.is_cuda:
            raise _lib.EmposeError('SensorFitter needs GPU tensors; there is no CPU fallback')
        net, dev, (B, F) = self.net, marker_pos.device, marker_pos.shape[:2]
        T, K = B * F, self.num_steps
        inputs = net._lgd_inputs(dev, B, F, marker_pos, marker_oris, offset_t, offset_r, marker_masks, seq_lengths, None)
        f32 = lambda t, w: None if t is None else t.to(device=dev, dtype=torch.float32).reshape(B, F, w).contiguous()
        pose_init, shape_init = (None, None) if init is None else (f32(init[0], 66), f32(init[1], 10))
        prior = f32(prior, 66)
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)
        out = {'pose': new(B, F, 66), 'shape': new(B, F, 10), 'joints': new(B, F, 66), 'pos': new(B, F, 36),
               'ori': new(B, F, 108), 'objective': new(K + 2, B), 'energy': new(B, F)}
        lib = _lib.lib()
        with torch.cuda.device(dev):
            handle = net._ensure_smpl_handle(dev)
            tgt = pack_sensor_inputs(inputs.marker_pos, inputs.marker_oris, net.marker_idxs).reshape(T, -1)
            io = _lib.FitIO()
            io.B, io.F, io.K = B, F, K
            io.tgt, io.ld_tgt = _lib.dptr(tgt), tgt.shape[1]
            for k in ('seq_lengths', 'marker_masks', 'offset_r', 'offset_t'):
                setattr(io, k, _lib.dptr(getattr(inputs, k)))
            io.pose_init, io.shape_init, io.pose_prior = _lib.dptr(pose_init), _lib.dptr(shape_init), _lib.dptr(prior)
            for k in ('lr', 'lr_decay', 'beta1', 'beta2', 'eps', 'lambda_pose', 'lambda_shape', 'lambda_smooth'):
                setattr(io, k, float(getattr(self, k)))
            io.shape_per_window, io.keep_best = int(self.shape_per_window), int(self.keep_best)
            for k, t in out.items():
                setattr(io, k, _lib.dptr(t))
            need = lib.empose_sensor_fit_workspace_bytes(handle, B, F)
            if self._workspace is None or self._workspace.numel() < need or self._workspace.device != dev:
                self._workspace = torch.empty(need, dtype=torch.uint8, device=dev)
            _lib.check(lib.empose_sensor_fit(handle, C.byref(io), _lib.dptr(self._workspace), self._workspace.numel(),
                                             _lib.current_stream()))
        return out

    @staticmethod
    def _init_of(init, sf, ef):
        """`init` as (pose (B,F,66), shape (B,F,10)): a pair, or a model's output dict (the polish use)."""
        if init is None:
            return None
        if isinstance(init, dict):
            pose = torch.cat([init['root_ori_hat'], init['pose_hat']], dim=-1)
            shape = init['shape_hat']
        else:
            pose, shape = init
        if shape.dim() == 2:
            shape = shape.unsqueeze(1).expand(shape.shape[0], pose.shape[1], shape.shape[-1])
        return pose[:, sf:ef], shape[:, sf:ef]

    def forward(self, batch, window_size=None, is_new_sequence=True, init=None):
        """The model interface: the four reference keys of `IterativeErrorFeedback.forward` plus `objective`
        ((K + 2, B) per window piece, concatenated along the batch axis)."""
        outs, sf = [], 0
        for batch_inputs in self.net.window_generator(batch, window_size=window_size):
            n = batch_inputs['marker_pos'].shape[1]
            res = self.fit_tensors(batch_inputs['marker_pos'], batch_inputs['marker_oris'], batch_inputs['offset_t'],
                                   batch_inputs['offset_r'], batch_inputs['marker_masks'], batch_inputs['seq_lengths'],
                                   init=self._init_of(init, sf, sf + n))
            outs.append(res)
            sf += n
        pose = _cat_windows([o['pose'] for o in outs])
        return {'pose_hat': pose[:, :, 3:], 'root_ori_hat': pose[:, :, :3],
                'shape_hat': _cat_windows([o['shape'] for o in outs]),
                'joints_hat': _cat_windows([o['joints'] for o in outs]),
                'objective': torch.cat([o['objective'] for o in outs], dim=1)}

    __call__ = forward
