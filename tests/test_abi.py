"""CPU-side checks of the boundary: the shared library builds/loads without a GPU and exports exactly the entry points
that include/empose_hip.h declares; the ctypes table mirrors the header; CPU tensors are refused (no fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from em_pose_amd import _lib
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, 'include', 'empose_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(empose_[a-z0-9_]+)\s*\(', text)))


def test_header_symbols_are_exported_and_bound():
    names = _declared()
    assert 'empose_lgd_forward' in names and 'empose_smpl_sensors_fwd_bwd' in names and len(names) >= 18
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n), 'library does not export ' + n
        assert n in _lib.SIGNATURES, 'ctypes table misses ' + n
    assert sorted(_lib.SIGNATURES) == names
    assert lib.empose_arch() == b'gfx950'


def test_struct_layouts_match_the_header_field_order():
    text = open(os.path.join(ROOT, 'include', 'empose_hip.h')).read()

    def fields(struct_name):
        end = re.search(r'\}\s*' + struct_name + ';', text).start()
        start = text.rfind('typedef struct {', 0, end) + len('typedef struct {')
        body = text[start:end]
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        out = []
        for decl in body.split(';'):
            decl = decl.strip()
            if not decl:
                continue
            for part in decl.split(','):
                name = re.findall(r'([A-Za-z_][A-Za-z0-9_]*)\s*(?:\[[^\]]*\])*\s*$', part.strip())
                out.append(name[0])
        return out
    for cname, cls in (('empose_smpl_desc', _lib.SmplDesc), ('empose_dense_desc', _lib.DenseDesc),
                       ('empose_mlp_desc', _lib.MlpDesc), ('empose_lstm_desc', _lib.LstmDesc),
                       ('empose_model_desc', _lib.ModelDesc), ('empose_lgd_io', _lib.LgdIO),
                       ('empose_mesh_desc', _lib.MeshDesc), ('empose_rnn_desc', _lib.RnnDesc)):
        assert fields(cname) == [f[0] for f in cls._fields_], cname


def test_bad_descriptors_are_rejected_without_a_gpu():
    lib = _lib.lib()
    desc = _lib.ModelDesc()
    handle = ctypes.c_void_p()
    assert lib.empose_model_create(ctypes.byref(desc), ctypes.byref(handle)) == -1
    assert b'n_sensors' in lib.empose_last_error()
    assert lib.empose_lgd_workspace_bytes(None, 4, 4) == 0


def test_model_workspace_queries_return_zero_for_a_null_handle():
    lib = _lib.lib()
    for T in (96, 0, -1):
        assert lib.empose_smpl_workspace_bytes(None, T) == 0
        assert lib.empose_update_workspace_bytes(None, T) == 0


def test_training_bookkeeping_calls_refuse_bad_arguments_without_a_gpu():
    """Every check of the loss and bookkeeping entry points (csrc/api_train.hip) precedes its launch: the calls below
    return an error before any GPU work, so the pointers only have to be non-NULL."""
    from em_pose_amd.helpers.configuration import CONSTANTS
    lib = _lib.lib()
    buf = np.zeros(64, np.float32)          # never read: every call below is refused
    p = ctypes.c_void_p(buf.ctypes.data)

    def loss_io(**change):
        io = _lib.LossIO()
        io.B, io.F, io.n_hist, io.n_markers = 2, 4, 3, 6
        for k, v in enumerate(CONSTANTS.S_CONFIG_6):
            io.marker_idx[k] = v
        for name, kind in _lib.LossIO._fields_:
            if kind is ctypes.c_void_p:
                setattr(io, name, p)
        io.ld_inputs = 72
        for k, v in change.items():
            if k == 'marker_idx':
                io.marker_idx[v[0]] = v[1]
            else:
                setattr(io, k, v)
        return io
    nbytes = lib.empose_lgd_losses_workspace_bytes(2, 4, 3)
    assert nbytes == 4 * 3 * 2 * 4 * 4 + 256
    for B, F, n in ((0, 4, 3), (2, 0, 3), (2, 4, 0), (-1, 4, 3)):
        assert lib.empose_lgd_losses_workspace_bytes(B, F, n) == 0

    def losses(io, ws=p, size=nbytes):
        return lib.empose_lgd_losses(ctypes.byref(io) if io is not None else None, ws, ctypes.c_size_t(size), None)
    assert losses(None) != 0 and losses(loss_io(), ws=None) != 0
    for name in ('pose_hist', 'shape_hist', 'markers_hist', 'markers_ori_hist', 'joints_final', 'pose_gt', 'shape_gt',
                 'inputs', 'd_pose', 'd_shape', 'd_markers', 'd_markers_ori', 'd_joints', 'loss_vals'):
        assert losses(loss_io(**{name: None})) == EMPOSE_EINVAL, name
    assert losses(loss_io(n_markers=5)) == EMPOSE_EINVAL
    assert losses(loss_io(marker_idx=(2, 12))) == EMPOSE_EINVAL and losses(loss_io(marker_idx=(0, -1))) == EMPOSE_EINVAL
    assert losses(loss_io(), size=nbytes - 1) != 0
    assert b'workspace' in lib.empose_last_error()
    assert losses(loss_io(ld_inputs=71)) == EMPOSE_EINVAL         # a short row would be read past its end
    assert b'ld_inputs' in lib.empose_last_error()
    assert losses(loss_io(n_markers=12, ld_inputs=143)) == EMPOSE_EINVAL

    def cotangent(F=4, d_pose=p, ld_g=66, ld_gb=10, dpad=p, dspad=p, Dp=p):
        return lib.empose_lgd_cotangent_step(2, F, 1, d_pose, p, p, p, p, ld_g, p, ld_gb, Dp, p, 0.1, 1, dpad, dspad, None)
    assert cotangent(F=1229) == EMPOSE_EINVAL      # 10 floats per frame above the 48 KB of dynamic shared memory
    assert cotangent(F=0) == EMPOSE_EINVAL and cotangent(d_pose=None) == EMPOSE_EINVAL and cotangent(Dp=None) == EMPOSE_EINVAL
    assert cotangent(ld_g=65) == EMPOSE_EINVAL and cotangent(ld_gb=9) == EMPOSE_EINVAL
    assert cotangent(dspad=None) == EMPOSE_EINVAL and cotangent(dpad=None) == EMPOSE_EINVAL
    assert lib.empose_lgd_additive_update(2, 4, 0.1, 1, p, p, p, None, p, p, None) == EMPOSE_EINVAL
    assert lib.empose_lgd_additive_update(0, 4, 0.1, 1, p, p, p, p, p, p, None) == EMPOSE_EINVAL
    assert lib.empose_window_mean(9, 4, 10, p, 10, p, 10, None) == EMPOSE_EINVAL       # T % F != 0
    assert lib.empose_window_mean(8, 4, 10, p, 9, p, 10, None) == EMPOSE_EINVAL
    assert lib.empose_window_mean(8, 4, 10, p, 10, p, 9, None) == EMPOSE_EINVAL
    assert lib.empose_window_mean(8, 4, 10, None, 10, p, 10, None) == EMPOSE_EINVAL
    assert lib.empose_axpby2d(3, 5, 1.0, p, 5, 1.0, p, 5, p, 4, None) == EMPOSE_EINVAL  # ldo < cols
    assert lib.empose_axpby2d(3, 5, 1.0, p, 4, 1.0, p, 5, p, 5, None) == EMPOSE_EINVAL
    assert lib.empose_axpby2d(3, 5, 1.0, p, 5, 1.0, p, 5, None, 5, None) == EMPOSE_EINVAL
    assert lib.empose_lgd_assemble_inputs(4, 72, p, 72, p, p, p, 72 + 75, None) == EMPOSE_EINVAL
    assert lib.empose_lgd_assemble_inputs(4, 72, p, 71, p, p, p, 224, None) == EMPOSE_EINVAL
    assert lib.empose_lgd_assemble_inputs(4, 72, p, 72, None, p, p, 224, None) == EMPOSE_EINVAL


def test_cpu_tensors_raise_instead_of_falling_back():
    from em_pose_amd.bodymodels.smpl import SMPLLayer
    from em_pose_amd.helpers.configuration import lgd_config
    from em_pose_amd.nn.models import create_model
    smpl = SMPLLayer(H.small_model())
    net = create_model(lgd_config(12, True, 2, hidden=32, rnn_hidden=32), smpl).eval()
    x = torch.zeros(1, 4, 36)
    with pytest.raises(_lib.EmposeError):
        net.forward_tensors(x, torch.zeros(1, 4, 108), torch.zeros(1, 12, 3), torch.eye(3).expand(1, 12, 3, 3))
    with pytest.raises(_lib.EmposeError):
        smpl(poses_body=torch.zeros(2, 63), betas=torch.zeros(2, 10))
    net.train()
    with pytest.raises(RuntimeError):  # the inference entry point refuses training mode ...
        net.forward_tensors(x, x, x, x)
    from em_pose_amd.data.data import SyntheticBatch
    w = {'poses': np.zeros((1, 4, 66), np.float32), 'shapes': np.zeros((1, 10), np.float32),
         'marker_pos': np.zeros((1, 4, 36), np.float32), 'marker_oris': np.zeros((1, 4, 108), np.float32),
         'offset_t': np.zeros((1, 12, 3), np.float32), 'offset_r': np.tile(np.eye(3, dtype=np.float32), (1, 12, 1, 1))}
    with pytest.raises(_lib.EmposeError):  # ... and the training path refuses CPU tensors as well
        net(SyntheticBatch(w))


EMPOSE_EINVAL = -1   # include/empose_hip.h

# Kernel-variant options and their defaults (EMPOSE_OPTIONS, csrc/options.h).
OPTION_DEFAULTS = {
    'mlp_fused': 1, 'lstm_persist': 1, 'gemm_splitk': 1, 'heads_rows': 1, 'lstm_seq': 0, 'bptt_wave': 1, 'gemm_wide': 1,
    'smpl_tile': 1, 'smpl_fuse': 1, 'train_fused': 0, 'atb_target': 0, 'atb_fast': 1, 'atb_chunk': 0,
    'mesh_skin_mfma': 0, 'train_epi': 1, 'spin_limit': 0, 'rows_x3': 1, 'lstm_x3': 1, 'train_cols': 1, 'cols_coop': 1,
    'mesh_x3': 1, 'train_x3': 1, 'lstm_midseq': 0, 'lstm_mid16': 1, 'lstm_mid_x3': 1, 'lstm_fewrows': 1, 'mlp_x3': 1,
}


def test_options_round_trip_reset_and_refuse_unknown_names():
    lib = _lib.lib()
    assert len(OPTION_DEFAULTS) == 27
    lib.empose_reset_options()
    try:
        for name, default in OPTION_DEFAULTS.items():
            assert lib.empose_get_option(name.encode()) == default, name
        for i, name in enumerate(OPTION_DEFAULTS):   # every name writes its own field: distinct values, read back after all
            assert lib.empose_set_option(name.encode(), 100 + i) == 0, name
        for i, name in enumerate(OPTION_DEFAULTS):
            assert lib.empose_get_option(name.encode()) == 100 + i, name
        assert lib.empose_reset_options() == 0
        for name, default in OPTION_DEFAULTS.items():
            assert lib.empose_get_option(name.encode()) == default, name
        assert lib.empose_set_option(b'no_such_option', 1) == EMPOSE_EINVAL
        assert lib.empose_last_error() == b"unknown option 'no_such_option'"
        assert lib.empose_get_option(b'no_such_option') == -1
        assert lib.empose_set_option(None, 1) == EMPOSE_EINVAL
        assert lib.empose_get_option(None) == -1
    finally:
        lib.empose_reset_options()
