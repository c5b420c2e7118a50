"""The two root-frame entry points at the C boundary: every refusal comes before any GPU work (so the refusals run
without a GPU too, on host buffers that are never read), and repeated launches give the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from em_pose_amd import _lib
from tests import normalize_root_ref as NR

EINVAL = -1
BOTH = NR.ROTATE | NR.SUBTRACT


def test_refusals_come_before_any_gpu_work():
    lib = _lib.lib()
    buf = np.zeros(4096, np.float32)   # host memory: a launch would fault, a refusal never touches it
    p = C.c_void_p(buf.ctypes.data)
    fwd = lambda T=8, seg=4, conv=0, root=p, ld=3, trans=p, ro=p, to=p, flags=BOTH: \
        lib.empose_root_frame_fwd(T, seg, conv, root, ld, trans, ro, to, flags, None)
    vjp = lambda T=8, seg=4, conv=0, root=p, ld=3, trans=p, dr=p, dt=p, gr=p, gt=p, flags=BOTH, ws=p, nb=4096: \
        lib.empose_root_frame_vjp(T, seg, conv, root, ld, trans, dr, dt, gr, gt, flags, ws, nb, None)
    for f in (fwd, vjp):
        assert f(root=None) == EINVAL                      # NULL required pointers
        assert f(trans=None) == EINVAL
        assert f(T=0) == EINVAL and f(T=-4) == EINVAL      # sizes
        assert f(seg=0) == EINVAL and f(seg=-1) == EINVAL
        assert f(T=9) == EINVAL                            # T % seg_len != 0
        assert b'multiple' in lib.empose_last_error()
        assert f(conv=2) == EINVAL and f(conv=-1) == EINVAL
        assert b'Rodrigues' in lib.empose_last_error()
        assert f(ld=2) == EINVAL
        assert f(flags=4) == EINVAL
    assert fwd(ro=None) == EINVAL and fwd(to=None) == EINVAL
    assert vjp(gr=None) == EINVAL and vjp(gt=None) == EINVAL
    assert vjp(dr=None, dt=None) == EINVAL                 # both cotangents NULL
    assert b'both NULL' in lib.empose_last_error()
    assert vjp(flags=0, trans=None) == EINVAL              # d_trans_out without a translation to differentiate
    assert vjp(ws=None) == EINVAL and vjp(nb=8) == EINVAL  # workspace


@pytest.mark.gpu
def test_repeated_launches_give_identical_bits():
    rng = np.random.default_rng(2)
    dev = 'cuda:0'
    for T, seg in ((4000, 1000), (4096, 32)):
        t = lambda: torch.from_numpy(rng.normal(0, 0.7, size=(T, 3)).astype(np.float32)).to(dev)
        root, trans, d_root, d_trans = t(), t(), t(), t()
        f0 = NR.run_fwd(root, trans, seg, 'smplx', BOTH)
        g0 = NR.run_vjp(root, trans, d_root, d_trans, seg, 'smplx', BOTH)
        for _ in range(3):
            f1 = NR.run_fwd(root, trans, seg, 'smplx', BOTH)
            g1 = NR.run_vjp(root, trans, d_root, d_trans, seg, 'smplx', BOTH)
            for a, b in zip(f0 + g0, f1 + g1):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
