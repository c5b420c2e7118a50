#!/usr/bin/env python
"""
Times the model-free sensor fit (em_pose_amd/nn/fitting.py, csrc/api_fit.hip, csrc/sensor_fit.hip): K = 50 steps, 12
sensors, zero init, on the V = 6890 synthetic body model, at 1024 windows of 32 frames and at 1 window of 256 frames:

  empose_sensor_fit  one call of the C ABI on readings that are already packed and on the device
  torch-driven loop  the same loop driven from Python on the same GPU: `empose_smpl_sensors_fwd_bwd` per iteration, then
                     float32 torch operations for the energies, J, the priors' gradients, Adam and keep-best.  This is
                     the yardstick: the tree had no fitter before this one
  evaluation x K     K calls of `empose_smpl_sensors_fwd_bwd` alone (forward + reverse), and
  fit_step x K       K calls of `empose_sensor_fit_step` alone: the share of an iteration the new kernel takes

Per row: 3 warm-up calls, then 10 timed calls, each measured with device events and with the host clock around the call
plus a final synchronisation; the medians are printed.  The table is measured three times in turn (rounds); the spread of
a median over the rounds is the run-to-run spread a difference has to exceed.  Before anything is timed the two loops
are compared (objective rows; their parameters drift apart as any two float32 Adam trajectories do).

    python scripts/dev/bench_sensor_fit.py [--out profiles/sensor_fit_mi355x.txt]
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from em_pose_amd import _lib, synthetic  # noqa: E402
from em_pose_amd.bodymodels.smpl import SMPLLayer  # noqa: E402
from em_pose_amd.nn.fitting import SensorFitter  # noqa: E402
from em_pose_amd.nn.models import pack_sensor_inputs  # noqa: E402

ROUNDS, K = 3, 50
HP = dict(lr=0.05, lr_decay=1.0, beta1=0.9, beta2=0.999, eps=1e-8, lambda_pose=1e-3, lambda_shape=1e-3, lambda_smooth=1.0)


def timed(fn, calls=10, warmup=3):
    ev, wall = [], []
    for it in range(warmup + calls):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if it >= warmup:
            ev.append(a.elapsed_time(b))
            wall.append((t1 - t0) * 1e3)
    return float(np.median(ev)), float(np.median(wall))


class Problem(object):
    """Readings of `synthetic.make_windows` on the device, packed, with every buffer the loops need."""

    def __init__(self, fitter, B, F, dev):
        self.fitter, self.B, self.F, self.T = fitter, B, F, B * F
        net = fitter.net
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)

        def sensors(poses, betas, o_r, o_t):
            pos, ori, _ = net.get_estimated_real_markers(up(poses), up(betas), up(o_r), up(o_t), frames_per_window=1)
            return pos.cpu().numpy(), ori.cpu().numpy()
        w = synthetic.make_windows(B, F, 77, sensors)
        self.marker_pos, self.marker_oris = up(w['marker_pos']), up(w['marker_oris'])
        self.offset_t, self.offset_r = up(w['offset_t']), up(w['offset_r'])
        self.tgt = pack_sensor_inputs(self.marker_pos, self.marker_oris, net.marker_idxs).reshape(self.T, -1)
        self.s = torch.ones(self.T, device=dev)
        self.handle = net._ensure_smpl_handle(dev)
        lib = _lib.lib()
        self.nbytes = lib.empose_smpl_workspace_bytes(self.handle, self.T)
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        z = lambda *shape: torch.zeros(*shape, device=dev)
        self.pos, self.ori, self.joints = z(B, F, 36), z(B, F, 108), z(B, F, 66)
        self.g_theta, self.g_beta = z(B, F, 66), z(B, F, 10)
        self.io = _lib.FitIO()
        self.io.B, self.io.F, self.io.K = B, F, K
        self.io.tgt, self.io.ld_tgt = _lib.dptr(self.tgt), self.tgt.shape[1]
        for k, v in HP.items():
            setattr(self.io, k, v)
        self.io.shape_per_window, self.io.keep_best = 1, 1
        self.step_bufs = [z(B, F, w) for w in (66, 10, 66, 66, 10, 10, 66, 10)] + [z(B), z(B), z(B, F, 66), z(B, F, 10)]
        self.step_bufs[9].fill_(float('inf'))

    def fit(self):
        return self.fitter.fit_tensors(self.marker_pos, self.marker_oris, self.offset_t, self.offset_r)

    def evaluate(self, theta, beta):
        p = _lib.dptr
        _lib.check(_lib.lib().empose_smpl_sensors_fwd_bwd(
            self.handle, self.T, self.F, p(theta), 66, p(beta), 10, p(self.offset_r), p(self.offset_t), p(self.tgt),
            self.tgt.shape[1], p(self.s), p(self.pos), p(self.ori), p(self.joints), p(self.g_theta), 66, p(self.g_beta),
            10, p(self.ws), self.nbytes, _lib.current_stream()))

    def step(self, k=0):
        p = _lib.dptr
        th, be, m_th, v_th, m_be, v_be, th1, be1, J, best_J, best_th, best_be = self.step_bufs
        _lib.check(_lib.lib().empose_sensor_fit_step(
            self.handle, C.byref(self.io), k, p(th), p(be), p(self.g_theta), p(self.g_beta), p(self.pos), p(self.ori),
            p(self.s), p(m_th), p(v_th), p(m_be), p(v_be), p(th1), p(be1), None, p(J), p(best_J), p(best_th), p(best_be),
            _lib.current_stream()))

    def torch_loop(self):
        """The yardstick.  Full windows, no missing sensors, 12 sensors: s = 1 and every frame is live."""
        B, F, T, dev = self.B, self.F, self.T, self.tgt.device
        lp, ls, lm = HP['lambda_pose'], HP['lambda_shape'], HP['lambda_smooth']
        b1, b2, eps = HP['beta1'], HP['beta2'], HP['eps']
        z = lambda *shape: torch.zeros(*shape, device=dev)
        theta, beta = z(B, F, 66), z(B, F, 10)
        m_th, v_th, m_be, v_be = z(B, F, 66), z(B, F, 66), z(B, 10), z(B, 10)
        best_J, best_th, best_be = torch.full((B,), float('inf'), device=dev), z(B, F, 66), z(B, F, 10)
        tgt_pos, tgt_ori = self.tgt[:, :36].reshape(B, F, 12, 3), self.tgt[:, 36:].reshape(B, F, 12, 9)
        rows = z(K + 2, B)

        def objective():
            e = (self.pos.reshape(B, F, 12, 3) - tgt_pos).norm(dim=-1).sum(-1) + \
                (self.ori.reshape(B, F, 12, 9) - tgt_ori).norm(dim=-1).sum(-1)
            d = theta[:, 1:] - theta[:, :-1]
            return e.sum(1) + 0.5 * lp * theta[:, :, 3:].square().sum((1, 2)) + 0.5 * lm * d.square().sum((1, 2)) + \
                0.5 * ls * beta[:, 0].square().sum(1)

        def keep(J):
            better = J < best_J
            best_th.copy_(torch.where(better[:, None, None], theta, best_th))
            best_be.copy_(torch.where(better[:, None, None], beta, best_be))
            best_J.copy_(torch.where(better, J, best_J))
        for k in range(K):
            self.evaluate(theta, beta)
            rows[k] = J = objective()
            keep(J)
            g = self.g_theta.clone()
            g[:, :, 3:] += lp * theta[:, :, 3:]
            d = theta[:, 1:] - theta[:, :-1]
            g[:, 1:] += lm * d
            g[:, :-1] -= lm * d
            gs = self.g_beta.sum(1) + ls * beta[:, 0]
            lr_k, c1, c2 = HP['lr'] * HP['lr_decay'] ** k, 1.0 / (1.0 - b1 ** (k + 1)), 1.0 / (1.0 - b2 ** (k + 1))
            m_th.mul_(b1).add_(g, alpha=1 - b1)
            v_th.mul_(b2).addcmul_(g, g, value=1 - b2)
            m_be.mul_(b1).add_(gs, alpha=1 - b1)
            v_be.mul_(b2).addcmul_(gs, gs, value=1 - b2)
            theta = theta - lr_k * (c1 * m_th) / ((c2 * v_th).sqrt() + eps)
            beta = (beta[:, 0] - lr_k * (c1 * m_be) / ((c2 * v_be).sqrt() + eps))[:, None].expand(B, F, 10).contiguous()
        self.evaluate(theta, beta)
        rows[K] = J = objective()
        keep(J)
        rows[K + 1] = best_J
        theta, beta = best_th, best_be
        self.evaluate(theta, beta)
        return {'pose': theta, 'shape': beta, 'objective': rows}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--out', default=None)
    args = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('needs an MI355X: a timing without the GPU says nothing')
    dev = torch.device('cuda:0')
    fitter = SensorFitter.from_smpl(SMPLLayer(synthetic.make_model()), 12, num_steps=K, **HP)
    fitter.net.to(dev).eval()
    lines = ['model-free sensor fit, K = {} steps, 12 sensors, zero init, keep-best, V = 6890, on {} ({}):'.format(
                 K, torch.cuda.get_device_name(0), torch.cuda.get_device_properties(0).gcnArchName),
             'median of 10 calls after 3 warm-up calls, milliseconds; median over {} rounds [lowest .. highest round]'.format(ROUNDS)]
    fmt = lambda x: '{:.3f} [{:.3f} .. {:.3f}]'.format(float(np.median(x)), min(x), max(x))
    for B, F in ((1024, 32), (1, 256)):
        pb = Problem(fitter, B, F, dev)
        ours, theirs = pb.fit()['objective'], pb.torch_loop()['objective']
        torch.cuda.synchronize()
        ratio_o, ratio_t = (ours[-1] / ours[0]).cpu().numpy(), (theirs[-1] / theirs[0]).cpu().numpy()
        first = float(((ours[0] - theirs[0]).abs() / theirs[0]).max())
        assert first <= 1e-5, first
        rows = (('empose_sensor_fit', pb.fit), ('torch-driven loop', pb.torch_loop),
                ('evaluation x K', lambda: [pb.evaluate(pb.step_bufs[0], pb.step_bufs[1]) for _ in range(K)]),
                ('fit_step x K', lambda: [pb.step(k) for k in range(K)]))
        res = {name: [] for name, _ in rows}
        for _ in range(ROUNDS):
            for name, fn in rows:
                res[name].append(timed(fn))
        lines += ['', '{} windows x {} frames ({} frames):'.format(B, F, B * F),
                  'returned J / J at the init over the windows: empose_sensor_fit {:.3f} .. {:.3f}, torch-driven loop {:.3f} .. '
                  '{:.3f}; J at the init, largest relative difference {:.1e}'.format(ratio_o.min(), ratio_o.max(), ratio_t.min(),
                                                                                  ratio_t.max(), first),
                  '{:<20} {:>30} {:>30}'.format('', 'events', 'wall')]
        for name, _ in rows:
            lines.append('{:<20} {:>30} {:>30}'.format(name, fmt([r[0] for r in res[name]]), fmt([r[1] for r in res[name]])))
        ev = {name: float(np.median([r[0] for r in res[name]])) for name, _ in rows}
        lines.append('per iteration: evaluation {:.1f} us, fit_step {:.1f} us ({:.1f} % of their sum); '
                     'torch-driven loop / empose_sensor_fit = {:.2f} (events)'.format(
                         ev['evaluation x K'] / K * 1e3, ev['fit_step x K'] / K * 1e3,
                         100.0 * ev['fit_step x K'] / (ev['fit_step x K'] + ev['evaluation x K']),
                         ev['torch-driven loop'] / ev['empose_sensor_fit']))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
