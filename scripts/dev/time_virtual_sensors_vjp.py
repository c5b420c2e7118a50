"""Dev: time the virtual sensors' vector-Jacobian product against the forward and against torch autograd through the
oracle.

At T frames (default 16384) of posed synthetic SMPL-H meshes (V = 6890), in interleaved rounds (clocks drift with
temperature and power state), median / min / max per call of:
  fwd 12              empose_virtual_sensors_fwd, the 12 model sensors
  vjp 12              empose_virtual_sensors_vjp, the 12 model sensors, cotangents on pos, ori and normals
  vjp normals         empose_virtual_sensors_vjp over the whole mesh (M = V, SMPLLayer.vertex_normals), normals only
  torch autograd 12   float32 torch autograd of oracle.torch_ref vertex_normals_sub + sensor_frames on the same GPU,
                      forward + backward, 12 sensors
  torch autograd nor  the same for vertex_normals_sub over the whole mesh, in chunks of 1024 frames
and the bytes each VJP has to move at the least, with the fraction of 8 TB/s that the median reaches.
"""
import statistics
import sys

sys.path.insert(0, '.')
import numpy as np
import torch

from em_pose_amd import _lib, synthetic
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.data.virtual_sensors import VirtualMarkerHelper
from em_pose_amd.helpers.configuration import CONSTANTS as CONST
from oracle import torch_ref as R

dev = 'cuda:0'
T = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
model = synthetic.make_model()
smpl = SMPLLayer(model).to(dev)
V = smpl.n_vertices
g = torch.Generator().manual_seed(3)
pose = (torch.randn(T, 63, generator=g) * 0.3).to(dev)
root = (torch.randn(T, 3, generator=g) * 0.3).to(dev)
betas = torch.randn(T, 10, generator=g).to(dev)
with torch.no_grad():
    verts, _ = smpl(poses_body=pose, betas=betas, poses_root=root)
helper = VirtualMarkerHelper(smpl)
ids12, ids_all = list(CONST.VERTEX_IDS), list(range(V))
lib = _lib.lib()


def setup(ids, cot_keys):
    """Tables, cotangents, output and workspace of one VJP case."""
    center, hel, deg, faces, max_deg = helper._tables(ids, verts.device)
    rev = helper._reverse_tables(ids, V, verts.device)
    M = len(ids)
    shapes = {'pos': (T, M, 3), 'ori': (T, M, 3, 3), 'nor': (T, M, 3)}
    cots = {k: (torch.randn(shapes[k], generator=g).to(dev) if k in cot_keys else None) for k in shapes}
    d_v = torch.empty(T, V, 3, device=dev)
    ws_bytes = lib.empose_virtual_sensors_vjp_workspace_bytes(T, M)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

    def run():
        _lib.check(lib.empose_virtual_sensors_vjp(T, V, _lib.dptr(verts), M, max_deg, _lib.dptr(center),
                                                  _lib.dptr(hel), _lib.dptr(deg), _lib.dptr(faces), rev[0].shape[0],
                                                  *[_lib.dptr(a) for a in rev[:7]], rev[7].shape[0],
                                                  _lib.dptr(rev[7]), _lib.dptr(cots['pos']),
                                                  _lib.dptr(cots['ori']), _lib.dptr(cots['nor']), _lib.dptr(d_v),
                                                  _lib.dptr(ws), ws_bytes, _lib.current_stream()))
    return run, cots, ws_bytes


vjp12, cots12, ws12 = setup(ids12, ('pos', 'ori', 'nor'))
vjp_nor, cots_nor, ws_nor = setup(ids_all, ('nor',))


def fwd12():
    helper._forward(verts, ids12)


def oracle_case(ids, with_frames, chunk):
    sub_faces, vf_sub, helpers = R.sensor_tables(model['f'], ids)
    sf, vf = torch.from_numpy(sub_faces).to(dev), torch.from_numpy(vf_sub).to(dev)
    cots = cots12 if with_frames else cots_nor

    def run():
        for t0 in range(0, T, chunk):
            sl = slice(t0, t0 + chunk)
            v = verts[sl].clone().requires_grad_(True)
            nor = R.vertex_normals_sub(v, sf, vf)
            outs, cot = [nor], [cots['nor'][sl]]
            if with_frames:
                outs += [v[:, ids], R.sensor_frames(v, nor, ids, helpers.tolist())]
                cot += [cots['pos'][sl], cots['ori'][sl]]
            torch.autograd.backward(outs, cot)
    return run


cases = [('fwd 12', fwd12, 20), ('vjp 12', vjp12, 20), ('vjp normals', vjp_nor, 10),
         ('torch autograd 12', oracle_case(ids12, True, T), 5), ('torch autograd nor', oracle_case(ids_all, False, 1024), 2)]
res = {name: [] for name, _, _ in cases}
for rnd in range(ROUNDS):
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
print('T = %d frames, V = %d, %d rounds, ms per call' % (T, V, len(res['vjp 12'])))
for name, _, _ in cases:
    r = res[name]
    print('  %-19s median %8.3f  min %8.3f  max %8.3f' % (name, statistics.median(r), min(r), max(r)))
m = {k: statistics.median(v) for k, v in res.items()}
# the least each VJP has to move: 12 sensors -- the dense d_vertices write (the cotangents and the few vertices read are
# negligible); whole mesh -- read vertices, d_normals, write d_vertices, write and read back the scratch rows once
dense = T * V * 3 * 4
need = {'vjp 12': dense + T * 12 * 15 * 4,
        'vjp normals': 3 * dense + 2 * T * V * 9 * 4}
for k, b in need.items():
    print('  %-12s %.2f GB at the least: %.2f TB/s, %.0f%% of 8 TB/s' % (k, b / 1e9, b / m[k] / 1e9, 100 * b / m[k] / 8e9))
print('  workspace: %.1f MB (12 sensors), %.1f MB (whole mesh)' % (ws12 / 2 ** 20, ws_nor / 2 ** 20))
print('  torch autograd 12 / vjp 12 = %.1f, torch autograd nor / vjp normals = %.1f' % (
    m['torch autograd 12'] / m['vjp 12'], m['torch autograd nor'] / m['vjp normals']))
