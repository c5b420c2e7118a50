"""
SMPLLayer under autograd: the full-mesh vector-Jacobian product (empose_mesh_vjp, csrc/mesh_vjp.hip and the reverse
kinematic chain in csrc/mesh_chain.hip) against float64 autograd through the oracle (oracle/torch_ref.py smpl_fk).

The bar, per frame row of g_poses, g_betas and g_trans separately: the largest error of the row is at most 1e-4 x the
row's largest |g64|, and at most 4 x the error of float32 CPU autograd through the same oracle (the control) plus
1e-7 x the row's scale.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from em_pose_amd import _lib, synthetic
from em_pose_amd.bodymodels import tables as TB
from em_pose_amd.bodymodels.smpl import SMPLLayer
from oracle import torch_ref as R
from tests import helpers as H

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def model():
    return synthetic.make_model()


def _inputs(rng, n, n_body=63, n_betas=10, with_trans=True, zero_frames=()):
    pose = rng.normal(0, 0.4, size=(n, n_body)).astype(np.float32)
    root = rng.normal(0, 0.5, size=(n, 3)).astype(np.float32)
    for f in zero_frames:
        pose[f] = 0
        root[f] = 0
    betas = rng.normal(0, 1, size=(n, n_betas)).astype(np.float32)
    trans = rng.normal(0, 1, size=(n, 3)).astype(np.float32) if with_trans else None
    return pose, root, betas, trans


def _oracle_grads(model, conv, dtype, pose, root, betas, trans, dv, dj):
    """(g_poses [n][66] (root first), g_betas [n][10], g_trans [n][3] or None) of autograd through the oracle."""
    bm = R.BodyModelTensors(model, dtype=dtype, rodrigues_convention=conv)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dtype).requires_grad_(True)
    pb, rt, bt = t(pose), t(root), t(betas)
    tr = t(trans) if trans is not None else None
    v, j = R.smpl_fk(bm, pb[:, :63], bt, rt, tr)
    loss = 0
    if dv is not None:
        loss = loss + (v * torch.from_numpy(dv).to(dtype)).sum()
    if dj is not None:
        loss = loss + (j * torch.from_numpy(dj).to(dtype)).sum()
    loss.backward()
    g_poses = torch.cat([rt.grad, pb.grad[:, :63]], dim=1).numpy().astype(np.float64)
    return g_poses, bt.grad[:, :10].numpy().astype(np.float64), (tr.grad.numpy().astype(np.float64) if tr is not None
                                                                 else None)


def _ours(smpl, pose, root, betas, trans, dv, dj):
    g = lambda a: torch.from_numpy(a).to(DEV).requires_grad_(True)
    pb, rt, bt = g(pose), g(root), g(betas)
    tr = g(trans) if trans is not None else None
    v, j = smpl(poses_body=pb, betas=bt, poses_root=rt, trans=tr)
    outs, cots = [], []
    if dv is not None:
        outs.append(v); cots.append(torch.from_numpy(dv).to(DEV))
    if dj is not None:
        outs.append(j); cots.append(torch.from_numpy(dj).to(DEV))
    torch.autograd.backward(outs, cots)
    g_poses = torch.cat([rt.grad, pb.grad[:, :63]], dim=1).cpu().numpy().astype(np.float64)
    return g_poses, bt.grad.cpu().numpy().astype(np.float64), (tr.grad.cpu().numpy().astype(np.float64)
                                                               if tr is not None else None)


def _check_rows(name, got, g64, g32):
    scale = np.abs(g64).max(axis=1)
    err = np.abs(got - g64).max(axis=1)
    err32 = np.abs(g32 - g64).max(axis=1)
    bad = np.nonzero((err > 1e-4 * scale) | (err > 4 * err32 + 1e-7 * scale))[0]
    assert bad.size == 0, '{}: rows {} err {} scale {} control {}'.format(
        name, bad[:8], err[bad[:8]], scale[bad[:8]], err32[bad[:8]])


def _check_against_oracle(model, smpl, conv, rng, n, with_trans=True, zero_frames=(), vertices=True, joints=True):
    V, nj = model['v_template'].shape[0], smpl.n_joints
    pose, root, betas, trans = _inputs(rng, n, with_trans=with_trans, zero_frames=zero_frames)
    dv = rng.normal(0, 1, size=(n, V, 3)).astype(np.float32) if vertices else None
    dj = rng.normal(0, 1, size=(n, nj, 3)).astype(np.float32) if joints else None
    got = _ours(smpl, pose, root, betas, trans, dv, dj)
    g64 = _oracle_grads(model, conv, torch.float64, pose, root, betas, trans, dv, dj)
    g32 = _oracle_grads(model, conv, torch.float32, pose, root, betas, trans, dv, dj)
    for name, a, b, c in zip(('g_poses', 'g_betas', 'g_trans'), got, g64, g32):
        if b is not None:
            _check_rows(name, a, b, c)
    return got


@pytest.mark.parametrize('conv', ['smplx', 'so3'])
def test_mesh_vjp_against_float64_autograd(model, conv):
    smpl = SMPLLayer(model, rodrigues_convention=conv).to(DEV)
    rng = np.random.default_rng(3)
    _check_against_oracle(model, smpl, conv, rng, 70, zero_frames=(0, 33, 69))


def test_mesh_vjp_partial_cotangents(model):
    smpl = SMPLLayer(model).to(DEV)
    rng = np.random.default_rng(4)
    _check_against_oracle(model, smpl, 'smplx', rng, 40, joints=False)    # d_joints NULL
    _check_against_oracle(model, smpl, 'smplx', rng, 40, vertices=False)  # d_vertices NULL (no vertex sweep)
    # through the module: 156 pose columns, 16 betas, poses_root and trans not given; the gradients land in the caller's
    # columns and shapes, zeros where the reference's would be zero
    n, V = 24, model['v_template'].shape[0]
    pose, _, betas, _ = _inputs(rng, n, n_body=156, n_betas=16)
    dv = rng.normal(0, 1, size=(n, V, 3)).astype(np.float32)
    dj = rng.normal(0, 1, size=(n, 52, 3)).astype(np.float32)
    zero_root = np.zeros((n, 3), np.float32)
    g64 = _oracle_grads(model, 'smplx', torch.float64, pose, zero_root, betas, None, dv, dj)
    for b_in in (betas, betas[:1], betas[0]):   # per frame, one broadcast row, a 1-D vector
        pb = torch.from_numpy(pose).to(DEV).requires_grad_(True)
        bt = torch.from_numpy(np.ascontiguousarray(b_in)).to(DEV).requires_grad_(True)
        v, j = smpl(poses_body=pb, betas=bt)
        torch.autograd.backward([v, j], [torch.from_numpy(dv).to(DEV), torch.from_numpy(dj).to(DEV)])
        assert pb.grad.shape == pb.shape and bt.grad.shape == bt.shape
        gp = pb.grad.cpu().numpy()
        assert not gp[:, 63:].any()
        want = g64[0][:, 3:] if b_in.shape[0] == n else None
        if want is not None:
            assert np.abs(gp[:, :63] - want).max() <= 1e-4 * np.abs(want).max()
        gb = bt.grad.cpu().numpy().reshape(-1, 16)
        assert not gb[:, 10:].any()
        if b_in.shape[0] == n:
            assert np.abs(gb[:, :10] - g64[1]).max() <= 1e-4 * np.abs(g64[1]).max()
        else:
            bb = np.broadcast_to(b_in.reshape(1, -1), (n, 16)).copy()
            r = _oracle_grads(model, 'smplx', torch.float64, pose, zero_root, bb, None, dv, dj)[1].sum(axis=0)
            assert np.abs(gb[0, :10] - r).max() <= 1e-4 * np.abs(r).max()
    # only the trans input requires grad
    tr = torch.zeros(n, 3, device=DEV, requires_grad=True)
    v, _ = smpl(poses_body=torch.from_numpy(pose).to(DEV), betas=torch.from_numpy(betas).to(DEV), trans=tr)
    v.backward(torch.from_numpy(dv).to(DEV))
    np.testing.assert_allclose(tr.grad.cpu().numpy(), dv.astype(np.float64).sum(axis=1), rtol=1e-5, atol=1e-3)


def test_mesh_vjp_ragged_sizes_and_many_bones():
    """1, 131 and 700 frames (not multiples of the 32-frame block; split and unsplit sweeps) on a body model whose
    vertices are skinned by up to six bones (the feat sweep's EXTRA path)."""
    model = dict(H.small_model())
    V = model['v_template'].shape[0]
    rng = np.random.default_rng(12)
    w = np.array(model['weights'], dtype=np.float64, copy=True)
    for v in range(0, V, 3):
        bones = rng.choice(22, size=6, replace=False)
        w[v] = 0
        w[v, bones] = rng.uniform(0.1, 1.0, size=6)
        w[v] /= w[v].sum()
    model['weights'] = w.astype(model['weights'].dtype)
    assert TB.build_full_mesh_tables(model)['kb'] == 6
    smpl = SMPLLayer(model).to(DEV)
    for n, with_trans in ((1, True), (131, False), (700, True)):
        _check_against_oracle(model, smpl, 'smplx', rng, n, with_trans=with_trans)


def test_mesh_vjp_deterministic_and_non_interfering(model):
    smpl = SMPLLayer(model).to(DEV)
    rng = np.random.default_rng(5)
    n, V = 300, model['v_template'].shape[0]
    pose, root, betas, trans = _inputs(rng, n)
    dv = torch.from_numpy(rng.normal(0, 1, size=(n, V, 3)).astype(np.float32)).to(DEV)
    dj = torch.from_numpy(rng.normal(0, 1, size=(n, 52, 3)).astype(np.float32)).to(DEV)
    plain = [torch.from_numpy(a).to(DEV) for a in (pose, betas, root, trans)]
    v0, j0 = smpl(*plain[:2], poses_root=plain[2], trans=plain[3])
    assert v0.grad_fn is None and j0.grad_fn is None
    grads = []
    for _ in range(2):
        ins = [a.clone().requires_grad_(True) for a in plain]
        v, j = smpl(ins[0], ins[1], poses_root=ins[2], trans=ins[3])
        assert v.grad_fn is not None
        assert torch.equal(v.detach(), v0) and torch.equal(j.detach(), j0)
        torch.autograd.backward([v, j], [dv, dj])
        grads.append([a.grad.clone() for a in ins])
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    with torch.no_grad():
        ins = [a.clone().requires_grad_(True) for a in plain]
        v, j = smpl(ins[0], ins[1], poses_root=ins[2], trans=ins[3])
        assert v.grad_fn is None and j.grad_fn is None
        assert torch.equal(v, v0)


def test_mesh_vjp_bf16x3_handle_and_workspace_check(model):
    rng = np.random.default_rng(6)
    n, V = 50, model['v_template'].shape[0]
    pose, root, betas, trans = _inputs(rng, n)
    dv = rng.normal(0, 1, size=(n, V, 3)).astype(np.float32)
    dj = rng.normal(0, 1, size=(n, 52, 3)).astype(np.float32)
    exact = _ours(SMPLLayer(model).to(DEV), pose, root, betas, trans, dv, dj)
    fast_layer = SMPLLayer(model, arithmetic='bf16x3').to(DEV)
    fast = _ours(fast_layer, pose, root, betas, trans, dv, dj)
    for a, b in zip(exact, fast):
        assert np.abs(a - b).max() <= 1e-6 * np.abs(a).max()
    # a workspace one byte short is refused before any GPU work
    lib = _lib.lib()
    handle = fast_layer._mesh_handle(torch.device(DEV))
    need = lib.empose_mesh_vjp_workspace_bytes(handle, n)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    p = torch.zeros(n, 66, device=DEV)
    b = torch.zeros(n, 10, device=DEV)
    d = torch.zeros(n, 52, 3, device=DEV)
    gp, gb = torch.empty_like(p), torch.empty_like(b)
    args = (handle, n, _lib.dptr(p), _lib.dptr(b), None, _lib.dptr(d), _lib.dptr(gp), _lib.dptr(gb), None, _lib.dptr(ws))
    assert lib.empose_mesh_vjp(*args, need - 1, _lib.current_stream()) == -1
    assert lib.empose_mesh_vjp(*args, need, _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(gp).all()
