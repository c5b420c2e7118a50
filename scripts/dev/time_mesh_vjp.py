"""Dev: time the full-mesh vector-Jacobian product against the forward and against torch autograd through the oracle.

At T frames (default 16384) of the synthetic SMPL-H model, in interleaved rounds (clocks drift with temperature and
power state), median / min / max per call of:
  fwd mesh_x3=0   SMPLLayer.forward on the fp32 MFMA kernel
  fwd default     SMPLLayer.forward with the default options
  vjp             empose_mesh_vjp with vertex and joint cotangents
  torch autograd  float32 torch autograd of oracle.torch_ref.body_model_forward on the same GPU, forward + backward,
                  in chunks of 256 frames (as the reference's own SMPLLayer.fk windows long inputs)
"""
import statistics
import sys

sys.path.insert(0, '.')
import numpy as np
import torch

from em_pose_amd import _lib, synthetic
from em_pose_amd.bodymodels.smpl import SMPLLayer
from oracle import torch_ref as R

dev = 'cuda:0'
T = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
model = synthetic.make_model()
smpl = SMPLLayer(model).to(dev)
V = smpl.n_vertices
g = torch.Generator().manual_seed(3)
pose = (torch.randn(T, 63, generator=g) * 0.3).to(dev)
root = (torch.randn(T, 3, generator=g) * 0.3).to(dev)
betas = torch.randn(T, 10, generator=g).to(dev)
trans = torch.randn(T, 3, generator=g).to(dev)
dv = torch.randn(T, V, 3, generator=g).to(dev)
dj = torch.randn(T, 52, 3, generator=g).to(dev)
lib = _lib.lib()
poses = torch.cat([root, pose], dim=1).contiguous()
handle = smpl._mesh_handle(torch.device(dev))
ws_bytes = lib.empose_mesh_vjp_workspace_bytes(handle, T)
ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
g_poses = torch.empty(T, 66, device=dev)
g_betas = torch.empty(T, 10, device=dev)
g_trans = torch.empty(T, 3, device=dev)
bm = R.BodyModelTensors(model)
for k in ('v_template', 'shapedirs', 'posedirs', 'J_regressor', 'weights'):
    setattr(bm, k, getattr(bm, k).to(dev))


def fwd(opt):
    def run():
        if opt is None:
            lib.empose_reset_options()
        else:
            _lib.check(lib.empose_set_option(b'mesh_x3', opt))
        smpl(poses_body=pose, betas=betas, poses_root=root, trans=trans)
    return run


def vjp():
    _lib.check(lib.empose_mesh_vjp(handle, T, _lib.dptr(poses), _lib.dptr(betas), _lib.dptr(dv), _lib.dptr(dj),
                                   _lib.dptr(g_poses), _lib.dptr(g_betas), _lib.dptr(g_trans), _lib.dptr(ws), ws_bytes,
                                   _lib.current_stream()))


CHUNK = 256   # frames per oracle call: in one call of 16384 frames its batched (N*V) 4x4 products faulted the GPU


def torch_autograd():
    for t0 in range(0, T, CHUNK):
        sl = slice(t0, t0 + CHUNK)
        ins = [t[sl].clone().requires_grad_(True) for t in (root, pose, betas, trans)]
        v, j = R.body_model_forward(bm, ins[0], ins[1], ins[2], None, ins[3])
        torch.autograd.backward([v, j], [dv[sl], dj[sl]])


cases = [('fwd mesh_x3=0', fwd(0), 10), ('fwd default', fwd(None), 10), ('vjp', vjp, 10), ('torch autograd', torch_autograd, 2)]
res = {name: [] for name, _, _ in cases}
for rnd in range(5):
    for name, fn, reps in cases:
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res[name].append(e0.elapsed_time(e1) / reps)
    print('round %d: %s' % (rnd, ', '.join('%s %.3f' % (k, v[-1]) for k, v in res.items())), flush=True)
lib.empose_reset_options()
print('T = %d frames, V = %d, %d rounds, ms per call' % (T, V, len(res['vjp'])))
for name, _, _ in cases:
    r = res[name]
    print('  %-15s median %8.3f  min %8.3f  max %8.3f' % (name, statistics.median(r), min(r), max(r)))
m = {k: statistics.median(v) for k, v in res.items()}
print('  vjp / fwd mesh_x3=0 = %.2f, torch autograd / vjp = %.1f' % (m['vjp'] / m['fwd mesh_x3=0'],
                                                                  m['torch autograd'] / m['vjp']))
