"""
Synthetic sensor sampling on the sensor sub-mesh, the parts that need no GPU: the sub-mesh topology and tables
(bodymodels/tables.py build_sub_mesh_tables, SMPLLayer.sub_mesh), the argument checks of empose_sample_sensors_fwd /
_vjp, the factory switches, and the host plan of SampleMarkersWithOffsets(on_device=True) against the torch path's draws.
"""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from em_pose_amd import _lib, synthetic
from em_pose_amd.bodymodels import tables as TB
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.data.transforms import SMPLFK, SampleMarkersWithOffsets, get_end_to_end_preprocess_fn
from em_pose_amd.helpers.configuration import CONSTANTS as CONST, lgd_config
from tests import helpers as H

EINVAL = -1   # EMPOSE_EINVAL (include/empose_hip.h)


def _small():
    return H.small_model(), [int(v) for v in H.load_case('train_lgdrnn12_n2')['meta']['vertex_ids']]


MODELS = {'small': (_small, 60, None), 'v6890': (lambda: (synthetic.make_model(), list(CONST.VERTEX_IDS)), 84, 72)}


@pytest.mark.parametrize('which', sorted(MODELS))
def test_sub_mesh_topology_is_the_full_meshs(which):
    make, n_needed, n_faces = MODELS[which]
    model, ids = make()
    needed, faces = TB.sub_mesh_vertices(model['f'], ids)
    sub_faces, vf_sub, helpers = TB.sensor_topology(model['f'], ids)
    assert len(needed) == n_needed and (n_faces is None or len(faces) == n_faces)
    assert np.all(np.diff(needed) > 0)
    want = np.unique(np.concatenate([np.asarray(ids), helpers, sub_faces.reshape(-1)]))
    assert np.array_equal(needed, want)
    assert np.array_equal(needed[faces], sub_faces)           # the incident faces, ascending face id, corner order kept
    assert faces.min() == 0 and faces.max() == len(needed) - 1
    local = np.searchsorted(needed, ids)
    sub_faces_l, vf_sub_l, helpers_l = TB.sensor_topology(faces, local.tolist())
    assert np.array_equal(needed[helpers_l], helpers)         # the same helper vertices ...
    assert np.array_equal(vf_sub_l, vf_sub)                   # ... and the same fan order, entry by entry
    assert np.array_equal(needed[sub_faces_l], sub_faces)
    if which == 'v6890':
        assert int((vf_sub >= 0).sum(axis=1).max()) == 6


@pytest.mark.parametrize('which', sorted(MODELS))
def test_sub_mesh_tables_are_gathered_rows_of_the_full_tables(which):
    model, ids = MODELS[which][0]()
    full, sub = TB.build_full_mesh_tables(model), TB.build_sub_mesh_tables(model, ids)
    needed, nv, V = sub['needed'], sub['n_vertices'], full['n_vertices']
    assert nv == len(needed) == MODELS[which][1] and sub['j_off'] == nv * 3
    assert sub['kb'] == full['kb'] and sub['n_joints'] == full['n_joints'] == 52
    assert sub['ncp'] == sub['wc'].shape[0] >= nv * 3 + 52 * 3 and sub['ncp'] % 4 == 0
    rows = (needed[:, None] * 3 + np.arange(3)[None]).reshape(-1)
    assert np.array_equal(sub['wc'][:nv * 3], full['wc'][rows])
    assert np.array_equal(sub['wc'][nv * 3:nv * 3 + 156], full['wc'][V * 3:V * 3 + 156])     # all joint rows
    assert not sub['wc'][nv * 3 + 156:].any()
    assert np.array_equal(sub['skin_idx'], full['skin_idx'][needed])
    assert np.array_equal(sub['skin_w'], full['skin_w'][needed])
    assert np.array_equal(sub['parents'], full['parents'])
    for k in ('wc', 'skin_idx', 'skin_w', 'parents'):
        assert sub[k].flags['C_CONTIGUOUS'] and sub[k].dtype == full[k].dtype, k
    assert set(full) | {'needed', 'faces'} == set(sub)


def test_sub_mesh_layer_object():
    model, ids = _small()
    smpl = SMPLLayer(model)
    sub = smpl.sub_mesh(ids)
    assert smpl.sub_mesh(list(ids)) is sub and smpl.sub_mesh(ids[:6]) is not sub     # cached per id tuple
    needed, faces = TB.sub_mesh_vertices(model['f'], ids)
    assert np.array_equal(sub.needed, needed) and sub.n_vertices == 60 and sub.n_joints == 52
    assert np.array_equal(sub.model['f'], faces) and np.array_equal(sub.faces.numpy(), faces)
    assert sub.faces.dtype == torch.int32
    assert sub.local_ids(ids) == np.searchsorted(needed, ids).tolist()
    outside = [v for v in range(model['v_template'].shape[0]) if v not in set(needed.tolist())]
    with pytest.raises(ValueError):
        sub.local_ids([ids[0], outside[0]])
    with pytest.raises(ValueError):
        sub.local_ids([10 ** 6])
    assert sub.rodrigues_convention == smpl.rodrigues_convention and sub.arithmetic == smpl.arithmetic
    assert SMPLLayer(model, rodrigues_convention='so3').sub_mesh(ids).rodrigues_convention == 'so3'
    with pytest.raises(_lib.EmposeError):       # no CPU fallback, as on the full layer
        sub(poses_body=torch.zeros(2, 63), betas=torch.zeros(2, 10))
    # the tables follow the parent's: a state dict with another template rebuilds them
    tables_before = sub._mesh_tables()
    sd = smpl.state_dict()
    sd['bm.v_template'] = sd['bm.v_template'] + 0.01
    smpl.load_state_dict(sd)
    assert smpl.tables_version == 1
    assert np.array_equal(sub.needed, needed)
    after = sub._mesh_tables()
    assert after is not tables_before and not np.array_equal(after['wc'], tables_before['wc'])
    assert np.array_equal(after['wc'][:180], TB.build_full_mesh_tables(smpl.model)['wc'][
        (needed[:, None] * 3 + np.arange(3)[None]).reshape(-1)])


def test_smplfk_keeps_its_default_and_takes_vertex_ids():
    assert SMPLFK(None).vertex_ids is None
    assert SMPLFK(None, vertex_ids=np.asarray([3, 1])).vertex_ids == (3, 1)


# ---- the C ABI refuses bad arguments before any GPU work -----------------------------------------------------------------
def test_sample_sensors_calls_refuse_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    buf = np.zeros(64, np.float32)          # never read: every call below is refused
    p = ctypes.c_void_p(buf.ctypes.data)
    W = _lib.SAMPLE_LOCAL_WINDOW

    def fwd(N=2, F=3, V=10, v=p, M=4, max_deg=6, tabs=(p, p, p, p), mode=W, local=p, r=p, outs=(p,) * 6):
        return lib.empose_sample_sensors_fwd(N, F, V, v, M, max_deg, *tabs, mode, local, r, *outs, None)

    ws_bytes = lib.empose_sample_sensors_vjp_workspace_bytes(6, 4)
    up = lambda floats: (floats * 4 + 255) // 256 * 256     # scratch (9), d_pos (3), d_ori (9) per (frame, sensor)
    assert ws_bytes == up(6 * 4 * 9) + up(6 * 4 * 3) + up(6 * 4 * 9)
    assert lib.empose_sample_sensors_vjp_workspace_bytes(4096, 12) == 4096 * 12 * 84
    for T, M in ((0, 4), (6, 0), (-1, 4)):
        assert lib.empose_sample_sensors_vjp_workspace_bytes(T, M) == 0

    def vjp(N=2, F=3, V=10, v=p, M=4, max_deg=6, tabs=(p, p, p, p), n_sub=5, rev=(p,) * 7, n_touched=7, touched=p,
            mode=W, local=p, r=p, cots=(p,) * 6, d_v=p, ws=p, size=ws_bytes):
        return lib.empose_sample_sensors_vjp(N, F, V, v, M, max_deg, *tabs, n_sub, *rev, n_touched, touched, mode,
                                             local, r, *cots, d_v, ws, ctypes.c_size_t(size), None)

    for call in (fwd, vjp):
        assert call(v=None) == EINVAL
        for i in range(4):
            assert call(tabs=tuple(None if j == i else p for j in range(4))) == EINVAL, i
        for name in ('N', 'F', 'V', 'M', 'max_deg'):
            assert call(**{name: 0}) == EINVAL and call(**{name: -3}) == EINVAL, name
        assert call(mode=3) == EINVAL and call(mode=-1) == EINVAL
        assert b'mode' in lib.empose_last_error()
        assert call(mode=_lib.SAMPLE_LOCAL_WINDOW, local=None) == EINVAL
        assert call(mode=_lib.SAMPLE_LOCAL_FRAME, local=None) == EINVAL
        assert b'local' in lib.empose_last_error()
    assert fwd(outs=(None,) * 6) == EINVAL and b'outputs' in lib.empose_last_error()
    assert vjp(cots=(None,) * 6) == EINVAL and b'cotangents' in lib.empose_last_error()
    assert vjp(d_v=None) == EINVAL and vjp(touched=None) == EINVAL
    for i in range(7):
        assert vjp(rev=tuple(None if j == i else p for j in range(7))) == EINVAL, i
    assert vjp(n_sub=0) == EINVAL and vjp(n_touched=0) == EINVAL
    assert vjp(ws=None) == EINVAL and vjp(size=ws_bytes - 1) == EINVAL
    assert b'workspace' in lib.empose_last_error()


# ---- the factory ---------------------------------------------------------------------------------------------------------
def _offset_sets():
    z = np.load(os.path.join(H.GOLDEN, 'preprocess.npz'))
    return [{k: z['offsets/%d/%s' % (i, k)] for k in ('means', 'covs', 'r', 'vertex_ids')} for i in range(3)]


def test_factory_switches_and_defaults():
    sets = _offset_sets()
    cfg = lgd_config(12, True, 2)
    fn = get_end_to_end_preprocess_fn(cfg, None, sets)
    assert fn.fk.vertex_ids is None and fn.sample_markers.on_device is False and fn.noise_fn is None
    assert SampleMarkersWithOffsets(None, sets).on_device is False
    fn = get_end_to_end_preprocess_fn(cfg, None, sets, device_offsets=True)
    assert fn.fk.vertex_ids is None and fn.sample_markers.on_device is True
    fn = get_end_to_end_preprocess_fn(cfg, None, sets, sensors_only=True)
    assert fn.fk.vertex_ids == tuple(int(v) for v in sets[-1]['vertex_ids']) and fn.sample_markers.on_device is False
    noisy = lgd_config(12, True, 2, suppression_noise_length=0.3, noise_num_markers=2, offset_noise_level=1)
    fn = get_end_to_end_preprocess_fn(noisy, None, sets, randomize_if_configured=True, device_normalize=True,
                                      device_noise=True, device_offsets=True, sensors_only=True)
    assert fn.noise_fn is not None and fn.sample_markers.on_device and fn.sample_markers.noise_level == 1
    assert fn.fk.vertex_ids == tuple(fn.sample_markers.vertex_ids)


# ---- the host plan against the torch path --------------------------------------------------------------------------------
class _FixedSensors(object):
    """Stands in for VirtualMarkerHelper on the CPU: fixed sensor readings, so the torch path runs without a GPU."""

    def __init__(self, t, m, seed):
        g = torch.Generator().manual_seed(seed)
        self.pos = torch.randn(t, m, 3, generator=g)
        self.ori = torch.linalg.qr(torch.randn(t, m, 3, 3, generator=g))[0].contiguous()
        self.nor = torch.randn(t, m, 3, generator=g)

    def get_virtual_pos_and_rot(self, vertices, vertex_ids):
        return self.pos, self.ori, self.nor


@pytest.mark.parametrize('level', [-1, 0, 1, 2, 3])
def test_host_plan_is_what_the_torch_path_draws(level):
    sets, n, f, m = _offset_sets(), 5, 4, 12
    host_path = SampleMarkersWithOffsets(None, sets, noise_level=level)
    twin = SampleMarkersWithOffsets(None, sets, noise_level=level, on_device=True)
    host_path.virtual_helper = sensors = _FixedSensors(n * f, m, seed=level + 7)
    drawn_sets = []
    for call in range(2):      # the offset-set draw advances from call to call, and so does torch's generator
        torch.manual_seed(1000 + level)
        if call:
            torch.randn(17)    # somewhere else in the stream
        state = torch.get_rng_state()
        batch = types.SimpleNamespace(batch_size=n, seq_length=f, vertices=torch.zeros(n, f, 6), vertices_subset=None)
        host_path(batch)
        after_host = torch.get_rng_state()
        torch.set_rng_state(state)
        means, r, local, mode = twin.plan(n, f)
        assert torch.equal(torch.get_rng_state(), after_host)     # both took the same draws from torch's global stream
        assert means.dtype == r.dtype == torch.float32
        assert torch.equal(means, batch.offset_t_augmented) and torch.equal(r, batch.offset_r_augmented)
        drawn_sets.append(means.clone())
        assert mode == {-1: _lib.SAMPLE_LOCAL_WINDOW, 0: _lib.SAMPLE_LOCAL_WINDOW, 1: _lib.SAMPLE_LOCAL_FRAME,
                        2: _lib.SAMPLE_LOCAL_NONE, 3: _lib.SAMPLE_LOCAL_NONE}[level]
        ori = sensors.ori.reshape(n, f, m, 3, 3)
        if mode == _lib.SAMPLE_LOCAL_NONE:
            assert local is None
            pos = sensors.pos.reshape(n, f, m, 3) + torch.matmul(ori, torch.zeros(n, f, m, 3, 1)).squeeze(-1)
        else:
            assert tuple(local.shape) == ((n, f, m, 3) if mode == _lib.SAMPLE_LOCAL_FRAME else (n, m, 3))
            assert (level == -1) == torch.equal(local, means)
            l = local if mode == _lib.SAMPLE_LOCAL_FRAME else local[:, None].expand(n, f, m, 3)
            pos = sensors.pos.reshape(n, f, m, 3) + torch.matmul(ori, l.to(ori.dtype).unsqueeze(-1)).squeeze(-1)
        assert torch.equal(pos.reshape(n, f, -1), batch.marker_pos_synth)          # the same draws, bit for bit
        assert torch.equal(torch.matmul(ori, r[:, None]).reshape(n, f, -1), batch.marker_ori_synth)
        if level == 3:
            assert torch.equal(r, torch.eye(3).expand(n, m, 3, 3))
    assert not torch.equal(drawn_sets[0], drawn_sets[1])     # RandomState(6273) moved on between the calls


def test_subset_without_a_sensors_fan_is_refused_before_any_launch():
    model, ids = _small()
    sets = _offset_sets()
    smpl = SMPLLayer(model)
    needed = smpl.sub_mesh(sets[-1]['vertex_ids']).needed
    for on_device in (False, True):
        tr = SampleMarkersWithOffsets(smpl, sets, on_device=on_device)
        batch = types.SimpleNamespace(batch_size=1, seq_length=2, vertices=torch.zeros(1, 2, (len(needed) - 1) * 3),
                                      vertices_subset=needed[:-1])
        with pytest.raises(ValueError, match='fans'):
            tr(batch)
        batch.vertices_subset = needed[::-1].copy()
        with pytest.raises(ValueError, match='ascending'):
            tr(batch)
        # the whole fan, in a larger subset with another numbering: accepted, ids by position
        wider = np.union1d(needed, [0, 1, 2, 159])
        helper, local = tr._helper_and_ids(types.SimpleNamespace(vertices_subset=wider))
        assert local == np.searchsorted(wider, tr.vertex_ids).tolist()
        assert np.array_equal(wider[np.asarray(helper.get_vertex_helpers(local))],
                              TB.sensor_topology(model['f'], tr.vertex_ids)[2])
