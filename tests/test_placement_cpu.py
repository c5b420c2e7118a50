"""
The sensor placement search without a GPU: the preconditions the GPU tests (tests/test_placement.py) rely on -- on their
scene the float64 definition (tests/placement_ref.py) finds the true sites with a wide gap at every number of frames --,
the identity that ties the score to the offset statistics, and every refusal -- bad arguments, CPU tensors -- before any
launch.
"""
import ctypes
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

from em_pose_amd import _lib
from em_pose_amd.data import placement as PL
from tests import helpers as H
from tests import offset_estimation_ref as REF
from tests import placement_ref as PREF

EINVAL = -1
FRAMES = (1, 2, 8, 40, 1300)


@pytest.fixture(scope='module')
def scene():
    """The scene of tests/test_offset_estimation.py: 1300 posed small-model meshes and noisy readings at the 12 ids."""
    faces, ids = np.asarray(H.small_model()['f'], dtype=np.int64), REF.small_ids()
    verts = REF.posed_small(1300, 62, ids=ids, min_cross=0.5)
    p, Rr, _, _ = REF.noisy_readings(verts, faces, ids, np.random.default_rng(61))
    return verts, faces, ids, p, Rr


def test_float64_definition_finds_the_true_sites_with_a_gap_of_two(scene):
    verts, faces, ids, p, Rr = scene
    smallest = np.inf
    for n in FRAMES:
        score, site, counts = PREF.scores(verts[:n], p[:n])
        assert site.tolist() == ids and counts.tolist() == [n] * 12, n
        gap = PREF.runner_up_gap(score)
        print('n {}: smallest second-best / best {:.2f}'.format(n, gap.min()))
        assert gap.min() >= 2.0, (n, gap)
        smallest = min(smallest, gap.min())
    assert smallest >= 2.0


def test_end_to_end_and_full_mesh_scenes_have_the_true_sites_in_float64():
    """The other two scenes of the GPU tests: the recordings `search_placement` is run on, pooled and per subject, and
    the 6890-vertex stand-in with readings along the sensor normals."""
    model, ids = H.small_model(), REF.small_ids()
    samples, subjects = PREF.recordings(model, ids, PREF.E2E_LAYOUT, PREF.E2E_SEED, offset_sd=PREF.E2E_OFFSET_SD)
    assert subjects == ['x', 'x', 'y'] and [s.n_frames for s in samples] == [150, 90, 130]
    v, p, masks = PREF.normalized_scene(model, samples)
    for name, sl in (('pooled', slice(0, 370)), ('x', slice(0, 240)), ('y', slice(240, 370))):
        score, site, counts = PREF.scores(v[sl], p[sl], masks[sl])
        gap = PREF.runner_up_gap(score).min()
        print('{}: smallest second-best / best {:.2f}'.format(name, gap))
        assert site.tolist() == ids and gap >= 2.0 and 0 < counts.min() < sl.stop - sl.start, name
    v, p, ids = PREF.full_mesh_scene()
    assert v.shape == (64, 6890, 3) and p.shape == (64, 12, 3)
    score, site, _ = PREF.scores(v, p)
    gap = PREF.runner_up_gap(score).min()
    print('full mesh: smallest second-best / best {:.2f}'.format(gap))
    assert site.tolist() == ids and gap >= 2.0


def test_score_is_what_the_offsets_pay_for_a_site(scene):
    verts, faces, ids, p, Rr = scene
    masks = (np.random.default_rng(5).uniform(size=(1300, 12)) > 0.05).astype(np.float32)
    for mk in (None, masks):
        score, site, counts = PREF.scores(verts, p, mk, candidates=sorted(ids))
        o, Q = REF.per_frame(verts, faces, ids, p, Rr, mk, torch.float64)
        st = REF.statistics(o, Q, mk, [(0, 1300)])
        assert np.array_equal(st['counts'][0], counts)
        want = PREF.moment_score(st['means'][0], st['covs'][0], counts)
        got = score[np.arange(12), np.searchsorted(sorted(ids), ids)]
        rel = np.abs(got - want) / want
        print('moment identity: largest relative difference {:.1e}'.format(rel.max()))
        assert rel.max() <= 1e-12


def test_reference_ties_masks_and_unread_sensors():
    rng = np.random.default_rng(9)
    v = rng.normal(size=(6, 5, 3))
    v[:, 3] = v[:, 1]                               # vertices 1 and 3 coincide in every frame
    p = v[:, [1, 4, 0]] + 0.01 * rng.normal(size=(6, 3, 3))
    masks = np.ones((6, 3), np.float32)
    masks[:, 2] = 0                                 # sensor 2: never read
    masks[:, 1] = 0
    masks[4, 1] = 1                                 # sensor 1: read in frame 4 alone
    score, site, counts = PREF.scores(v, p, masks)
    assert site.tolist() == [1, 4, -1] and counts.tolist() == [6, 1, 0]
    assert score[0, 1] == score[0, 3] and np.isinf(score[2]).all()
    assert score[1, 4] == ((p[4, 1] - v[4, 4]) ** 2).sum()
    score, site, _ = PREF.scores(v, p, masks, candidates=[0, 3, 4])
    assert site.tolist() == [3, 4, -1] and score.shape == (3, 3)


def test_bad_arguments_are_refused_before_any_launch():
    lib = _lib.lib()
    buf = np.zeros(4096, np.float32)   # host memory: a launch would fault, a refusal never touches it
    p = ctypes.c_void_p(buf.ctypes.data)
    T, V, M = 100, 160, 12

    def accumulate(T=T, V=V, M=M, C=None, cand='none', nbytes=1 << 24, **null):
        a = dict(vertices=p, p=p, masks=None, sums=p, counts=p, ws=p, dev=p)
        a.update(null)
        if isinstance(cand, str):
            host, dev, c = None, None, V
        else:
            table = np.ascontiguousarray(cand, dtype=np.int32)
            host, dev, c = ctypes.c_void_p(table.ctypes.data), a['dev'], len(table)
        if 'host' in null:
            host = null['host']
        return lib.empose_placement_accumulate(T, V, a['vertices'], M, a['p'], a['masks'], c if C is None else C, host, dev,
                                               a['sums'], a['counts'], a['ws'], nbytes, None)
    for name in ('vertices', 'p', 'sums', 'counts'):
        assert accumulate(**{name: None}) == EINVAL, name
    for bad in (dict(T=0), dict(V=0), dict(M=0), dict(C=0), dict(T=-1), dict(C=-3)):
        assert accumulate(**bad) == EINVAL, bad
    assert accumulate(T=2 ** 28, M=8) == EINVAL and b'T * M' in lib.empose_last_error()
    assert accumulate(M=2 ** 16, V=2 ** 15) == EINVAL and b'M * C' in lib.empose_last_error()
    assert accumulate(T=64 * 65535 + 1, M=1) == EINVAL and b'slabs' in lib.empose_last_error()
    assert accumulate(C=V - 1) == EINVAL and b'without a candidate list' in lib.empose_last_error()
    for cand, word in (([3, 2], b'ascend'), ([3, 3], b'ascend'), ([0, 5, 4, 7], b'ascend'), ([-1, 2], b'outside'),
                       ([0, V], b'outside'), ([V + 5], b'outside')):
        assert accumulate(cand=cand) == EINVAL, cand
        assert word in lib.empose_last_error(), (cand, lib.empose_last_error())
    assert accumulate(cand=[1, 2, 3], dev=None) == EINVAL and b'host and its device' in lib.empose_last_error()
    assert accumulate(cand=[1, 2, 3], host=None) == EINVAL
    need = lib.empose_placement_workspace_bytes(T, M, V)
    assert need >= 2 * M * V * 8 and lib.empose_placement_workspace_bytes(64, M, V) < need
    assert lib.empose_placement_workspace_bytes(65, 1, 1) >= 2 * 8
    for bad in ((0, M, V), (T, 0, V), (T, M, 0), (-1, M, V)):
        assert lib.empose_placement_workspace_bytes(*bad) == 0
    assert accumulate(nbytes=need - 1) == EINVAL and b'workspace' in lib.empose_last_error()
    assert accumulate(ws=None) == EINVAL

    def finish(M=M, C=V, **null):
        a = dict(sums=p, counts=p, cand=None, score=p, best=p, best_score=p)
        a.update(null)
        return lib.empose_placement_finish(M, C, a['sums'], a['counts'], a['cand'], a['score'], a['best'], a['best_score'],
                                           None)
    for name in ('sums', 'counts', 'score', 'best', 'best_score'):
        assert finish(**{name: None}) == EINVAL, name
    assert finish(M=0) == EINVAL and finish(C=0) == EINVAL and finish(M=2 ** 16, C=2 ** 15) == EINVAL


def test_cpu_tensors_are_refused():
    from em_pose_amd.bodymodels.smpl import SMPLLayer
    v, pos = torch.zeros(4, 160, 3), torch.zeros(4, 12, 3)
    with pytest.raises(_lib.EmposeError, match='no CPU fallback'):
        PL.placement_scores(v, pos, None)
    with pytest.raises(_lib.EmposeError, match='no CPU fallback'):
        PL.placement_scores(v, pos, torch.ones(4, 12), candidates=[1, 2])
    with pytest.raises(_lib.EmposeError, match='no CPU fallback'):
        PL.placement_finish(torch.zeros(12, 160, dtype=torch.float64), torch.zeros(12, dtype=torch.int32))
    sample = types.SimpleNamespace(marker_pos_real=np.zeros((4, 36), np.float32))
    with pytest.raises(_lib.EmposeError, match='no CPU fallback'):
        PL.search_placement(SMPLLayer(H.small_model()), [sample])
    with pytest.raises(ValueError, match='at least one recording'):
        PL.search_placement(SMPLLayer(H.small_model()), [])


def test_candidates_excluding_bones_on_the_small_model():
    model = H.small_model()
    owner = np.argmax(np.asarray(model['weights']), axis=1)
    n_joints = model['weights'].shape[1]
    everything = PL.candidates_excluding_bones(model, [])
    assert everything.dtype == np.int32 and everything.tolist() == list(range(160))
    bones = [int(b) for b in np.unique(owner)[:3]]
    kept = PL.candidates_excluding_bones(model, bones)
    assert 0 < len(kept) < 160 and (np.diff(kept) > 0).all()
    assert not np.isin(owner[kept], bones).any() and np.isin(owner[np.setdiff1d(np.arange(160), kept)], bones).all()
    from em_pose_amd.bodymodels.smpl import SMPLLayer
    assert np.array_equal(PL.candidates_excluding_bones(SMPLLayer(model), bones), kept)     # a layer or its arrays
    assert len(PL.candidates_excluding_bones(model, range(n_joints))) == 0
    with pytest.raises(ValueError, match='bones'):
        PL.candidates_excluding_bones(model, [n_joints])
    with pytest.raises(ValueError, match='candidates'):
        PL.Candidates(np.zeros(0, np.int32), 'cpu')
    with pytest.raises(ValueError, match='int32'):
        PL.Candidates([0, 2 ** 31], 'cpu')


def test_script_parses_with_and_without_the_new_flags():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts', 'estimate_offsets.py')
    spec = importlib.util.spec_from_file_location('estimate_offsets_script', path)
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    args = script.arg_parser().parse_args(['--synthetic', '--out', 'somewhere'])
    assert args.synthetic and args.out == 'somewhere' and not args.search_placement and not args.exclude_hands
    assert args.recordings is None and args.device == 'cuda:0' and args.subject_from_id is None
    args = script.arg_parser().parse_args(['--recordings', 'd', '--out', 'o', '--search_placement', '--exclude_hands'])
    assert args.search_placement and args.exclude_hands and args.recordings == 'd'
