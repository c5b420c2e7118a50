"""CPU checks of empose_mesh_vjp's argument validation: every refusal happens before any GPU work, so it is testable
without a device."""
import ctypes

from em_pose_amd import _lib

EINVAL = -1


def test_mesh_vjp_rejects_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)   # stands in for device pointers: never dereferenced on these paths
    handle_buf = ctypes.create_string_buffer(512)
    fake_handle = ctypes.cast(handle_buf, ctypes.c_void_p)

    def call(handle, T, dv, dj, poses=p, betas=p, g_poses=p, g_betas=p):
        return lib.empose_mesh_vjp(handle, T, poses, betas, dv, dj, g_poses, g_betas, None, p, 1 << 20, None)

    assert call(None, 4, p, p) == EINVAL
    assert b'null' in lib.empose_last_error()
    assert call(fake_handle, 4, p, p, poses=None) == EINVAL
    assert call(fake_handle, 4, p, p, betas=None) == EINVAL
    assert call(fake_handle, 4, p, p, g_poses=None) == EINVAL
    assert call(fake_handle, 4, p, p, g_betas=None) == EINVAL
    assert call(fake_handle, 0, p, p) == EINVAL
    assert b'T must be positive' in lib.empose_last_error()
    assert call(fake_handle, -3, p, None) == EINVAL
    assert call(fake_handle, 4, None, None) == EINVAL
    assert b'both NULL' in lib.empose_last_error()
    assert lib.empose_mesh_vjp_workspace_bytes(None, 4) == 0
