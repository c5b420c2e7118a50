"""Root normalisation, the checks that need no GPU: the ctypes table, the fixture recorded from the reference against a
float64 restatement written here, and the default NormalizeRoot, which must keep its numbers."""
import ctypes as C
import hashlib
import types

import numpy as np
import torch

from em_pose_amd import _lib
from em_pose_amd.data.transforms import NormalizeRoot, matrix_to_rotvec
from em_pose_amd.eval.metrics import rotvec_to_matrix
from tests import normalize_root_ref as NR


def test_signatures_of_the_root_frame_entry_points():
    sig = _lib.SIGNATURES
    assert sig['empose_root_frame_fwd'] == (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                       C.c_void_p, C.c_void_p, C.c_int, C.c_void_p])
    assert sig['empose_root_frame_vjp_workspace_bytes'] == (C.c_size_t, [C.c_int, C.c_int])
    res, args = sig['empose_root_frame_vjp']
    assert res is C.c_int and len(args) == 14 and args[-3:] == [C.c_void_p, C.c_size_t, C.c_void_p]
    lib = _lib.lib()   # header and table agree: tests/test_abi.py compares the two name lists
    assert lib.empose_root_frame_vjp_workspace_bytes(1000, 1000) == 768      # 16 waves x 9 floats, rounded to 256 bytes
    assert lib.empose_root_frame_vjp_workspace_bytes(64, 32) == 256
    assert lib.empose_root_frame_vjp_workspace_bytes(65, 64) == 0            # not a multiple


def test_fixture_is_self_consistent():
    fx = NR.load_fixture()
    a, b = fx['a'], fx['b']
    assert a['poses_root'].shape == (40, 3) and b['poses_root'].shape == (1, 3)
    # the restatement in float64 against the reference's functions in float64: same maps, so equal to rounding; the
    # reference's acos-based logarithm is accurate to ~1e-16 / sin(angle) in float64, angles up to 2.6 rad
    root64, trans64, Rn = NR.normalize64(a['poses_root'], a['trans'], 40, 'so3')
    ang = np.linalg.norm(root64, axis=1)
    assert ang[0] == 0.0 and 2.55 < ang.max() <= 2.6 + 1e-6
    assert np.abs(root64 - a['root64']).max() < 1e-12
    assert np.abs(trans64 - a['trans64']).max() < 1e-12
    # the recorded bar is the reference's float32 error against those values, and is of float32 size
    assert a['err_root'] == np.abs(a['root32'].astype(np.float64) - a['root64']).max()
    assert a['err_trans'] == np.abs(a['trans32'].astype(np.float64) - a['trans64']).max()
    assert 1e-8 < a['err_trans'] < 1e-5 and 1e-8 < a['err_root'] < 1e-5
    assert a['joints'].shape == (40, 52, 3) and a['vertices'].shape[0] == 40 and str(a['error']) == ''
    # one frame: the reference's squeeze collapses trans to (3,) and its body model refuses it; the meaning is zeros (1,3)
    assert b['trans32'].shape == (3,) and b['trans64'].shape == (1, 3) and not b['trans64'].any()
    assert 'RuntimeError' in str(b['error']) and not b['root64'].any()
    # the differentiable restatement (exact maps) agrees with the guarded one: the guards act below 0.01 rad only
    out, t = NR.normalize_torch(torch.from_numpy(a['poses_root']).double(), torch.from_numpy(a['trans']).double(), 40)
    assert np.abs(out.numpy() - root64).max() < 1e-7 and np.abs(t.numpy() - trans64).max() < 1e-7


def test_default_normalize_root_keeps_its_numbers():
    """The host path is the default and did not change: bit-equal to the float64 host computation it has always been
    (the transform before `on_device` existed, restated: rotations in float64, R_0^T R, the host logarithm, one cast)."""
    rng = np.random.default_rng(11)
    poses = torch.from_numpy(rng.normal(0, 0.7, size=(5, 9, 66)).astype(np.float32))
    trans = torch.from_numpy(rng.normal(0, 1, size=(5, 9, 3)).astype(np.float32))
    batch = NormalizeRoot()(types.SimpleNamespace(poses=poses.clone(), trans=trans.clone()))
    assert not batch.trans.any() and torch.equal(batch.trans_source, trans)
    assert torch.equal(batch.root_pose_source, poses[:, :, :3]) and torch.equal(batch.poses[:, :, 3:], poses[:, :, 3:])
    assert not batch.poses[:, 0, :3].any()
    Rm = rotvec_to_matrix(poses[:, :, :3].numpy().astype(np.float64))
    want = torch.from_numpy(matrix_to_rotvec(np.swapaxes(Rm[:, :1], -1, -2) @ Rm)).to(poses)
    assert torch.equal(batch.poses[:, :, :3], want)
    # a digest of the same output, recorded from the commit before this feature (float64 libm, then one rounding)
    assert hashlib.sha256(batch.poses.numpy().tobytes()).hexdigest() == \
        'b53c1d54a569ff55f03cfd02a2708b1646bc64dc126d3101222fe59a5bf9be07'
