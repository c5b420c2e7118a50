"""
Sensor placement search in HIP (csrc/placement.hip, em_pose_amd/data/placement.py) against the float64 restatement
(tests/placement_ref.py), on the 160-vertex scene of tests/test_offset_estimation.py unless said otherwise.

The bar of the scores, 1e-6 relative at every element against float64 evaluated on the same fp32 inputs: the kernel rounds
the difference, three squares, two adds, the division and the fp32 output -- about seven roundings of 2^-24, 4.2e-7 -- and
carries every sum over frames in double.  (The float32 CPU control measured 2.1e-7 at one frame and 5.9e-8 at 1300.)
The sites must equal the float64 argmin without exception: tests/test_placement_cpu.py holds the float64 gap between the
best and the second-best score at 2 x or more on every scene used here, against a bar of 1e-6.
"""
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from em_pose_amd import synthetic
from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.data import placement as PL
from tests import helpers as H
from tests import offset_estimation_ref as REF
from tests import placement_ref as PREF

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
BAR = 1e-6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = lambda a, dtype=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


@pytest.fixture(scope='module')
def scene():
    """1300 posed small-model meshes with noisy readings at the 12 ids, on the host and on the device; masks with 5 % of
    missing readings, a sensor that is never read and one that is read in frame 700 alone."""
    faces, ids = np.asarray(H.small_model()['f'], dtype=np.int64), REF.small_ids()
    verts = REF.posed_small(1300, 62, ids=ids, min_cross=0.5)
    p, _, _, _ = REF.noisy_readings(verts, faces, ids, np.random.default_rng(61))
    masks = (np.random.default_rng(63).uniform(size=(1300, 12)) > 0.05).astype(np.float32)
    masks[:, 3] = 0.0
    masks[:, 5] = 0.0
    masks[700, 5] = 1.0
    return dict(ids=ids, verts=verts, p=p, masks=masks, verts_d=gpu(verts), p_d=gpu(p), masks_d=gpu(masks))


def _search(verts_d, p_d, masks_d, slab, candidates=None):
    """One group in slabs of `slab` frames: (score, best, best_score, counts) on the host, and the device sums."""
    sums = counts = None
    cand = PL.Candidates.of(candidates, DEV)
    for at in range(0, verts_d.shape[0], slab):
        sl = slice(at, at + slab)
        sums, counts = PL.placement_scores(verts_d[sl], p_d[sl], None if masks_d is None else masks_d[sl], sums, counts,
                                           cand)
    score, best, best_score = PL.placement_finish(sums, counts, cand)
    return score.cpu().numpy(), best.cpu().numpy(), best_score.cpu().numpy(), counts.cpu().numpy(), sums


def _check(name, got, verts, p, masks=None, candidates=None):
    """Every score within the bar of float64, the sites the float64 argmin, exact counts, best_score the site's score."""
    score, best, best_score, counts, _ = got
    want, site, n = PREF.scores(verts, p, masks, candidates)
    assert score.shape == want.shape and score.dtype == np.float32 and best.dtype == np.int32
    assert np.array_equal(counts, n), name
    read = n > 0
    assert np.isposinf(score[~read]).all() and (best[~read] == -1).all() and np.isposinf(best_score[~read]).all(), name
    rel = np.abs(score[read].astype(np.float64) - want[read]) / want[read]
    print('{}: largest relative error {:.2e} (bar {:.0e})'.format(name, rel.max() if rel.size else 0.0, BAR))
    assert np.isfinite(score[read]).all() and (rel <= BAR).all(), (name, float(rel.max()))
    assert np.array_equal(best, site), (name, best, site)
    ids = np.arange(verts.shape[1]) if candidates is None else np.asarray(candidates)
    for m in np.nonzero(read)[0]:
        assert best_score[m] == score[m, np.searchsorted(ids, best[m])], (name, m)
    return want


# ---- 1. scores and sites against float64 ----------------------------------------------------------------------------------
@pytest.mark.parametrize('t', [1, 2, 63, 64, 65, 255, 256, 257, 1300])
def test_scores_and_sites_at_the_frame_counts_around_the_chunk(scene, t):
    got = _search(scene['verts_d'][:t], scene['p_d'][:t], None, 1024)
    _check('T {}'.format(t), got, scene['verts'][:t], scene['p'][:t])
    assert got[1].tolist() == scene['ids']          # and the float64 argmin is the true site (tests/test_placement_cpu.py)


@pytest.mark.parametrize('t,slab', [(257, 1), (257, 64), (1300, 64), (1300, 256), (1300, 1024)])
def test_slab_sizes_agree_within_the_bar(scene, t, slab):
    got = _search(scene['verts_d'][:t], scene['p_d'][:t], scene['masks_d'][:t], slab)
    want = _check('T {} slab {}'.format(t, slab), got, scene['verts'][:t], scene['p'][:t], scene['masks'][:t])
    whole = _search(scene['verts_d'][:t], scene['p_d'][:t], scene['masks_d'][:t], t)
    read = np.isfinite(want[:, 0])
    rel = np.abs(got[0][read].astype(np.float64) - whole[0][read]) / whole[0][read]
    print('slab {} against one slab of {}: largest relative difference {:.2e}'.format(slab, t, rel.max()))
    assert (rel <= BAR).all() and np.array_equal(got[1], whole[1]) and np.array_equal(got[3], whole[3])


@pytest.mark.parametrize('m', [1, 5, 12])
@pytest.mark.parametrize('cand', ['all', 'list37', 'single'])
def test_sensor_counts_and_candidate_lists(scene, m, cand):
    t, ids = 257, scene['ids']
    rng = np.random.default_rng(7)
    if cand == 'all':
        candidates = None
    elif cand == 'list37':        # the m sites and vertices drawn around them, ascending
        others = rng.choice(np.setdiff1d(np.arange(160), ids), 37 - m, replace=False)
        candidates = np.sort(np.concatenate([ids[:m], others])).astype(np.int32)
        assert len(candidates) == 37
    else:
        candidates = np.asarray([ids[0]], dtype=np.int32)
    got = _search(scene['verts_d'][:t], scene['p_d'][:t, :m].contiguous(), scene['masks_d'][:t, :m].contiguous(), 64,
                  candidates)
    _check('M {} {}'.format(m, cand), got, scene['verts'][:t], scene['p'][:t, :m], scene['masks'][:t, :m], candidates)


def test_one_vertex_mesh(scene):
    t = 65
    verts = np.ascontiguousarray(scene['verts'][:t, 9:10])
    got = _search(gpu(verts), scene['p_d'][:t], None, 64)
    _check('one vertex', got, verts, scene['p'][:t])
    assert got[0].shape == (12, 1) and (got[1] == 0).all()


# ---- 2. masks -------------------------------------------------------------------------------------------------------------
def test_unread_sensors_single_frames_and_what_masked_readings_hold(scene):
    verts, p, masks = scene['verts'], scene['p'], scene['masks']
    got = _search(scene['verts_d'], scene['p_d'], scene['masks_d'], 1024)
    _check('masks', got, verts, p, masks)
    score, best, best_score, counts, sums = got
    assert counts[3] == 0 and counts[5] == 1 and counts.tolist() == masks.sum(axis=0).astype(int).tolist()
    assert np.isposinf(score[3]).all() and best[3] == -1 and np.isposinf(best_score[3])
    one = ((p[700, 5].astype(np.float64) - verts[700].astype(np.float64)) ** 2).sum(axis=-1)   # frame 700 alone
    assert (np.abs(score[5] - one) <= BAR * one).all()
    # what a reading holds where it does not count changes nothing, not even NaN
    junk = p.copy()
    junk[masks == 0] = np.nan
    again = _search(scene['verts_d'], gpu(junk), scene['masks_d'], 1024)
    assert torch.equal(again[4], sums) and np.array_equal(again[0], score) and np.array_equal(again[1], best)


# ---- 3. exact ties --------------------------------------------------------------------------------------------------------
def test_coinciding_vertices_give_equal_bits_and_the_lower_id(scene):
    t = 130
    verts = scene['verts'][:t].copy()
    verts[:, 70] = verts[:, 20]
    verts[:, 150] = verts[:, 20]
    verts[:, 4] = verts[:, 99]
    rng = np.random.default_rng(11)
    p = (verts[:, [20, 99, 4, 150]] + rng.normal(0, 0.005, (t, 4, 3))).astype(np.float32)
    for candidates, want in ((None, [20, 4, 4, 20]), (np.asarray([4, 70, 99, 150], np.int32), [70, 4, 4, 70])):
        score, best, best_score, _, _ = got = _search(gpu(verts), gpu(p), None, 64, candidates)
        _check('tie', got, verts, p, None, candidates)
        col = (lambda v: v) if candidates is None else (lambda v: int(np.searchsorted(candidates, v)))
        assert np.array_equal(score[:, col(70)], score[:, col(150)]) and np.array_equal(score[:, col(4)], score[:, col(99)])
        if candidates is None:
            assert np.array_equal(score[:, 20], score[:, 70])
        assert best.tolist() == want


# ---- 4. determinism and independence ------------------------------------------------------------------------------------
def test_same_bits_again_alone_and_beside_garbage(scene):
    a, b = slice(0, 300), slice(300, 700)
    first = _search(scene['verts_d'][b], scene['p_d'][b], scene['masks_d'][b], 256)
    again = _search(scene['verts_d'][b], scene['p_d'][b], scene['masks_d'][b], 256)
    assert torch.equal(first[4], again[4]) and np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])
    # after another group, and on its own copies of its frames
    _search(scene['verts_d'][a], scene['p_d'][a], scene['masks_d'][a], 256)
    alone = _search(scene['verts_d'][b].clone(), scene['p_d'][b].clone(), scene['masks_d'][b].clone(), 256)
    assert torch.equal(first[4], alone[4]) and np.array_equal(first[0], alone[0])
    # garbage in the frames of the other groups
    verts_d, p_d, masks_d = scene['verts_d'].clone(), scene['p_d'].clone(), scene['masks_d'].clone()
    verts_d[a] = float('nan')
    p_d[a] = 1e30
    masks_d[a] = 1.0
    verts_d[700:] = float('inf')
    p_d[700:] = float('nan')
    beside = _search(verts_d[b], p_d[b], masks_d[b], 256)
    assert torch.equal(first[4], beside[4]) and np.array_equal(first[0], beside[0]) and np.array_equal(first[3], beside[3])


# ---- 5. end to end --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def recordings():
    model, ids = H.small_model(), REF.small_ids()
    samples, subjects = PREF.recordings(model, ids, PREF.E2E_LAYOUT, PREF.E2E_SEED, offset_sd=PREF.E2E_OFFSET_SD)
    return SMPLLayer(model).to(DEV), ids, samples, subjects


def test_search_placement_finds_the_sites_pooled_and_per_subject(recordings):
    smpl, ids, samples, subjects = recordings
    before = [(s.marker_pos_real.copy(), s.smpl_poses.copy()) for s in samples]
    with warnings.catch_warnings():
        warnings.simplefilter('error')       # nothing to warn about
        pooled = PL.search_placement(smpl, samples, subjects=subjects, slab=100)
        each = PL.search_placement(smpl, samples, subjects=subjects, per_subject=True, slab=64)
    for s, (p0, q0) in zip(samples, before):
        assert np.array_equal(s.marker_pos_real, p0) and np.array_equal(s.smpl_poses, q0)
    assert list(pooled) == ['all'] and list(each) == ['x', 'y']
    masks = np.concatenate([s.marker_masks for s in samples])
    for key, found, sl in (('all', pooled['all'], slice(0, 370)), ('x', each['x'], slice(0, 240)), ('y', each['y'], slice(240, 370))):
        assert found['vertex_ids'].tolist() == ids and found['vertex_ids'].dtype == np.int64, key
        assert np.array_equal(found['counts'], masks[sl].sum(axis=0).astype(np.int32)), key
        assert found['score'].shape == (12, 160) and found['score'].dtype == np.float32
        order = np.argsort(found['score'], axis=1, kind='stable')
        assert np.array_equal(found['runner_up_ids'], order[:, 1]) and (found['runner_up_ids'] != found['vertex_ids']).all()
        rms = 1e3 * np.sqrt(np.take_along_axis(found['score'], order[:, :2], axis=1))
        assert np.allclose(found['rms_mm'], rms[:, 0], rtol=1e-6) and np.allclose(found['runner_up_rms_mm'], rms[:, 1], rtol=1e-6)
        # 1 cm offsets and 5 mm of noise per axis: the rms at the site is a centimetre or two, the next vertex much further
        assert (found['rms_mm'] > 5.0).all() and (found['rms_mm'] < 60.0).all(), (key, found['rms_mm'])
        assert (found['runner_up_rms_mm'] >= np.sqrt(2.0) * found['rms_mm']).all(), key
    # a subject gives the same bits alone as after another
    alone = PL.search_placement(smpl, [samples[2]], slab=64)['all']
    assert np.array_equal(alone['score'], each['y']['score']) and np.array_equal(alone['vertex_ids'], each['y']['vertex_ids'])


def test_search_placement_candidates_and_warnings(recordings):
    smpl, ids, samples, subjects = recordings
    keep = PL.candidates_excluding_bones(smpl, [])
    assert keep.tolist() == list(range(160))
    some = np.sort(np.concatenate([ids, [0, 1, 2, 159]])).astype(np.int32)
    found = PL.search_placement(smpl, samples, candidates=some, slab=128)['all']
    assert found['vertex_ids'].tolist() == ids and found['score'].shape == (12, len(some))
    assert np.isin(found['runner_up_ids'], some).all()
    whole = PL.search_placement(smpl, samples, slab=128)['all']
    assert np.array_equal(found['score'], whole['score'][:, some])        # a candidate's sums do not depend on the list
    # a sensor that is never read, and two sensors with the same readings: warnings, no failure
    s = samples[2].extract_window(0, 64)
    s.marker_masks = s.marker_masks.copy()
    s.marker_masks[:, 2] = 0
    pos = s.marker_pos_real.reshape(64, 12, 3).copy()
    pos[:, 7] = pos[:, 4]
    s.marker_pos_real = pos.reshape(64, -1)
    with pytest.warns(UserWarning) as caught:
        found = PL.search_placement(smpl, [s])['all']
    text = ' | '.join(str(w.message) for w in caught)
    assert 'sensors [2] were read in no frame' in text and 'more than one sensor' in text and str(ids[4]) in text
    assert found['vertex_ids'][2] == -1 and found['counts'][2] == 0 and np.isposinf(found['rms_mm'][2])
    assert found['runner_up_ids'][2] == -1 and found['vertex_ids'][7] == found['vertex_ids'][4] == ids[4]


# ---- 6. the full-size mesh ------------------------------------------------------------------------------------------------
def test_full_size_mesh(scene):
    verts, p, ids = PREF.full_mesh_scene()
    want, site, _ = PREF.scores(verts, p)
    assert site.tolist() == ids                          # the precondition, also held by tests/test_placement_cpu.py
    score, best, best_score, counts, _ = _search(gpu(verts), gpu(p), None, 64)
    rel = np.abs(score.astype(np.float64) - want) / want
    print('full mesh: largest relative error {:.2e}'.format(rel.max()))
    assert (rel <= BAR).all() and counts.tolist() == [64] * 12
    gap = np.sort(want, axis=1)
    decided = gap[:, 1] - gap[:, 0] > 2e-6 * gap[:, 0]
    assert decided.all() and np.array_equal(best[decided], site[decided])
    hands_off = PL.candidates_excluding_bones(synthetic.make_model(), range(22, 52))       # a gathered candidate list
    assert 0 < len(hands_off) < 6890
    part = _search(gpu(verts), gpu(p), None, 64, hands_off)
    assert np.array_equal(part[0], score[:, hands_off])


# ---- 7. the script --------------------------------------------------------------------------------------------------------
def _run_script(out_dir, *flags):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    done = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'estimate_offsets.py'), '--synthetic', '--out',
                           str(out_dir), '--device', DEV] + list(flags), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=env, cwd=ROOT, timeout=600)
    assert done.returncode == 0, done.stderr.decode()[-2000:]
    return done.stdout.decode()


def test_script_searches_the_placement_and_writes_the_found_sites(tmp_path):
    printed = _run_script(tmp_path, '--search_placement')
    rows = re.findall(r'^\s+(\d+)\s+(\d+)\s+(-?\d+)\s+([\d.]+)\s+(-?\d+)\s+([\d.]+|inf)\s+(same|was \d+)\s*$', printed, re.M)
    assert [int(r[0]) for r in rows] == list(range(12)), printed
    sites = [int(r[2]) for r in rows]
    from em_pose_amd.helpers.configuration import CONSTANTS
    for r, default in zip(rows, CONSTANTS.VERTEX_IDS):
        assert r[6] == ('same' if int(r[2]) == default else 'was {}'.format(default))
        assert float(r[3]) <= float(r[5])
    assert sorted(os.listdir(str(tmp_path))) == ['synthA_offsets.npz', 'synthB_offsets.npz']
    for name in ('synthA', 'synthB'):
        z = np.load(str(tmp_path / (name + '_offsets.npz')))
        assert z['vertex_ids'].tolist() == sites and z['means'].shape == (12, 3)
        assert '{}: '.format(name) in printed


def test_script_without_the_flag_prints_what_it_printed_before(tmp_path):
    """The stdout of `--synthetic --out DIR`, recorded on an MI355X before the search existed
    (tests/golden/estimate_offsets_synthetic_stdout.txt, the output directory written as {OUT})."""
    printed = _run_script(tmp_path)
    want = open(os.path.join(ROOT, 'tests', 'golden', 'estimate_offsets_synthetic_stdout.txt')).read()
    assert printed.replace(str(tmp_path), '{OUT}') == want
