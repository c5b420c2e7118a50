"""CPU checks of empose_virtual_sensors_vjp's argument validation: every refusal happens before any GPU work, so it is
testable without a device."""
import ctypes

from em_pose_amd import _lib

EINVAL = -1


def test_virtual_sensors_vjp_rejects_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)   # stands in for device pointers: never dereferenced on these paths
    big = 1 << 20

    def call(T=4, V=10, M=3, max_deg=6, n_sub_faces=8, n_touched=5, vertices=p, tables=(p,) * 12, d_pos=p, d_ori=p,
             d_nor=p, d_vertices=p, ws=p, ws_bytes=big):
        (center, helper, deg, faces, sub_faces, face_ptr, face_sensors, vf_ptr, vf_corner, vs_ptr, vs_role,
         touched) = tables
        return lib.empose_virtual_sensors_vjp(T, V, vertices, M, max_deg, center, helper, deg, faces, n_sub_faces,
                                              sub_faces, face_ptr, face_sensors, vf_ptr, vf_corner, vs_ptr, vs_role,
                                              n_touched, touched, d_pos, d_ori, d_nor, d_vertices, ws, ws_bytes, None)

    assert call(vertices=None) == EINVAL
    assert b'null' in lib.empose_last_error()
    for i in range(12):   # every table
        tables = [p] * 12
        tables[i] = None
        assert call(tables=tuple(tables)) == EINVAL
        assert b'null' in lib.empose_last_error()
    assert call(d_vertices=None) == EINVAL
    for bad in (dict(T=0), dict(T=-2), dict(V=0), dict(M=0), dict(M=-1), dict(max_deg=0), dict(n_sub_faces=0),
                dict(n_touched=0)):
        assert call(**bad) == EINVAL
        assert b'sizes must be positive' in lib.empose_last_error()
    assert call(d_pos=None, d_ori=None, d_nor=None) == EINVAL
    assert b'all NULL' in lib.empose_last_error()
    assert call(ws=None) == EINVAL
    assert b'workspace too small' in lib.empose_last_error()
    need = lib.empose_virtual_sensors_vjp_workspace_bytes(4, 3)
    assert need > 0
    assert call(ws_bytes=need - 1) == EINVAL
    assert b'workspace too small' in lib.empose_last_error()


def test_virtual_sensors_vjp_workspace_bytes():
    lib = _lib.lib()
    ws = lib.empose_virtual_sensors_vjp_workspace_bytes
    for T, M in ((0, 12), (-1, 12), (16, 0), (16, -3)):
        assert ws(T, M) == 0
    assert ws(1, 12) >= 12 * 9 * 4
    assert ws(100, 12) >= 100 * 12 * 9 * 4
    # bounded: slabs of frames, whatever T (16384-frame slabs for few sensors, a 128 MB cap for many)
    assert ws(16384, 12) == ws(10 ** 6, 12)
    assert ws(10 ** 6, 6890) == ws(16384, 6890) <= (128 << 20) + 4096
    assert ws(10 ** 6, 10 ** 6) >= 10 ** 6 * 9 * 4   # at least one frame
