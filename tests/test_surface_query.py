"""
Point-to-mesh queries in HIP (csrc/surface_query.hip, em_pose_amd/eval/surface_metrics.py) against the float64 restatement
(tests/surface_query_ref.py), at every element of every case of `gpu_cases()`.

The tolerance is `surface_query_ref.TOL_M` = 7e-7 m (scaled for the 100 m query): four times the largest difference
between the restatement's float32 and float64 runs over these very inputs, 1.52e-7 m in the distance and 1.68e-7 m in the
closest point (tests/test_surface_query_cpu.py measures them).

Check (b), the closest point, is held against the float64 closest point ON THE FACE THE KERNEL REPORTS, and check (c)
holds that face's float64 distance to the float64 minimum: together they put `closest` within the tolerance of a nearest
point of the mesh.  Against "the" nearest point it cannot be held at every element, because the nearest point of a mesh is
not unique on its medial axis (the centre of the cube has six, half a metre apart, and the kernel's choice among faces
whose float64 distances differ by less than the tolerance is legitimately its own).  Wherever it IS unique -- every face
whose float64 distance is within the tolerance of the minimum has its float64 closest point within the tolerance of the
float64 argmin's -- `closest` is also held to that point, the literal form of the check.
Exact ties go to the lowest face id: at the centroid of the regular tetrahedron all four float32 d^2 have the same bits
(each face's closest point holds the same three coordinate values in another order and with other signs, and the
arithmetic is IEEE throughout), at the centre of the cube twelve faces tie, and a copy of a face ties with the face.
"""
import numpy as np
import pytest
import torch

from em_pose_amd.bodymodels.smpl import SMPLLayer
from em_pose_amd.eval import surface_metrics as SM
from tests import helpers as H
from tests import surface_query_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ULP = 2.0 ** -23
gpu = lambda a, dtype=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)
CASES = {c[0]: c[1:] for c in R.gpu_cases()}


def query(vertices, faces, points, mask=None, inside=True):
    out = SM.closest_point_on_mesh(gpu(vertices), faces, gpu(points), None if mask is None else gpu(mask), inside=inside)
    return SM.SurfaceResult(*[None if x is None else x.cpu().numpy() for x in out])


def same_bits(a, b, rows=slice(None)):
    return all(x is None or np.array_equal(x[rows], y, equal_nan=True) for x, y in zip(a, b))


@pytest.fixture(scope='module')
def launched():
    """Every case queried once, with the inside flag."""
    return {name: query(v, f, p) for name, (v, f, p) in CASES.items()}


# ---- 1. every element against float64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(CASES))
def test_every_element_against_float64(name, launched):
    vertices, faces, points = CASES[name]
    got = launched[name]
    t, q = points.shape[:2]
    assert got.dist.shape == (t, q) and got.face.dtype == np.int32 and got.bary.shape == (t, q, 3)
    assert got.closest.shape == (t, q, 3) and got.inside.dtype == bool
    pick = np.arange(q)
    for k in range(t):
        ref = R.closest_point(vertices[k], faces, points[k])
        tol = R.tolerance(points[k])
        face = got.face[k].astype(np.int64)
        assert ((face >= 0) & (face < len(faces))).all()
        err = np.abs(got.dist[k].astype(np.float64) - ref['dist'])
        print(name, k, 'dist %.3g closest %.3g of %.3g' % ((err / tol).max() * R.TOL_M, (np.abs(
            got.closest[k] - ref['all_closest'][pick, face]).max(axis=1) / tol).max() * R.TOL_M, R.TOL_M))
        assert (err <= tol).all(), (name, k, err.max())                                              # (a)
        on_face = ref['all_closest'][pick, face]
        assert (np.abs(got.closest[k] - on_face).max(axis=1) <= tol).all(), (name, k)                # (b)
        near = ref['all_dist'] - ref['dist'][:, None] <= tol[:, None]                                # (b), literally, where
        apart = np.abs(ref['all_closest'] - ref['closest'][:, None]).max(axis=2) > tol[:, None]      # the point is unique
        unique = ~(near & apart).any(axis=1)
        assert (np.abs(got.closest[k] - ref['closest']).max(axis=1)[unique] <= tol[unique]).all(), (name, k)
        assert unique.sum() >= (q + 1) // 2 or name in ('tetrahedron_centroid',), (name, k, int(unique.sum()))
        assert (ref['all_dist'][pick, face] - ref['dist'] <= tol).all(), (name, k)                   # (c)
        bary = got.bary[k].astype(np.float64)
        assert (got.bary[k] >= 0).all() and (np.abs(bary.sum(axis=1) - 1.0) <= 4 * ULP).all()        # (d)
        corners = vertices[k].astype(np.float64)[faces[face]]
        assert (np.abs(np.einsum('qc,qcd->qd', bary, corners) - got.closest[k]).max(axis=1) <= tol).all()
        assert all(np.isfinite(x[k]).all() for x in (got.dist, got.bary, got.closest))
        assert np.array_equal(got.inside[k], R.inside(vertices[k], faces, points[k])), (name, k)


def test_queries_on_a_vertex_an_edge_and_a_face_are_at_distance_zero(launched):
    for name in ('triangle', 'cube', 'degenerate'):
        got = launched[name]
        assert got.dist[0, :3].tolist() == [0.0, 0.0, 0.0], name
        assert np.array_equal(got.closest[0, :3], CASES[name][2][0, :3]), name
    assert launched['triangle'].bary[0, :3].tolist() == [[1, 0, 0], [0.5, 0.5, 0], [0.25, 0.25, 0.5]]
    far = launched['cube'].dist[0, 4]
    assert abs(far - np.sqrt(59.0 ** 2 + 80.0 ** 2 + 99.0 ** 2)) < 1e-4                # the 100 m query: corner (1, 0, 1)


def test_exact_ties_go_to_the_lowest_face_id(launched):
    centroid = launched['tetrahedron_centroid']                                        # all four faces tie, bit for bit
    assert centroid.face[0, 0] == 0
    assert abs(float(centroid.dist[0, 0]) - 0.5 / np.sqrt(3.0)) < R.TOL_M
    v, f = R.cube()
    got = query(v[None], f, np.full((1, 1, 3), 0.5, np.float32))                       # the centre: all twelve faces at 0.5
    assert got.dist[0, 0] == 0.5 and got.face[0, 0] == 0
    v, f = R.degenerate_mesh()
    assert (launched['degenerate'].face != len(f) - 1).all()                           # face 0 beats its copy
    both = query(v[None], f[[len(f) - 1, 0]], CASES['degenerate'][2][:, :5])
    assert (both.face[0, :3] == 0).all()


# ---- 2. masked queries ------------------------------------------------------------------------------------------------------
def test_masked_queries_hold_nan_and_reach_nothing(launched):
    for name in ('icosahedron', 'torus516', 'tetrahedron'):
        vertices, faces, points = CASES[name]
        t, q = points.shape[:2]
        mask = (np.random.default_rng(31).uniform(size=(t, q)) > 0.4).astype(np.float32)
        mask[0, 0] = 0.0
        mask[t - 1] = 0.0                                                              # a frame that does not count at all
        if q > 24:
            mask[0, 12:24] = 0.0                                                       # and a whole block of 12 queries
        dirty = points.copy()
        dirty[mask == 0] = np.nan
        got = query(vertices, faces, dirty, mask)
        off = mask == 0
        assert np.isposinf(got.dist[off]).all() and (got.face[off] == -1).all() and not got.inside[off].any()
        assert (got.bary[off] == 0).all() and (got.closest[off] == 0).all()
        for part, whole in zip(got, launched[name]):
            assert np.array_equal(part[~off], whole[~off]), name


# ---- 3. the same bits, whatever else is in the launch ---------------------------------------------------------------------
def test_same_bits_again_alone_and_beside_other_frames_and_queries(launched):
    for name in ('icosahedron', 'torus516'):
        vertices, faces, points = CASES[name]
        first = launched[name]
        assert same_bits(first, query(vertices, faces, points)), name
        for k in range(vertices.shape[0]):                                             # a frame alone
            assert same_bits(first, query(vertices[k:k + 1], faces, points[k:k + 1]), slice(k, k + 1)), (name, k)
        for cut in (slice(0, 1), slice(5, 12), slice(12, 13)):                         # queries alone, across the block of 12
            alone = query(vertices, faces, points[:, cut])
            assert all(np.array_equal(x[:, cut], y) for x, y in zip(first, alone)), (name, cut)
        plain = query(vertices, faces, points, inside=False)                           # without the inside test
        assert plain.inside is None and same_bits(first[:4], plain[:4]), name


def test_surface_distance_equals_the_one_shot_query_for_every_slab():
    smpl = SMPLLayer(H.small_model()).to(DEV)
    rng = np.random.default_rng(41)
    t = 7
    poses = gpu(rng.normal(0, 0.3, size=(t, 63)))
    root = gpu(rng.normal(0, 0.3, size=(t, 3)))
    betas = gpu(rng.normal(0, 1.0, size=(1, 10)))
    vertices, _ = smpl(poses_body=poses, betas=betas, poses_root=root)
    points = vertices[:, ::13][:, :12] + gpu(rng.normal(0, 0.01, size=(t, 12, 3)))
    mask = gpu((rng.uniform(size=(t, 12)) > 0.2).astype(np.float32))
    want = SM.closest_point_on_mesh(vertices, smpl.faces, points, mask, inside=True)
    for slab in (1, 3, 1024):
        got = smpl.surface_distance(points.reshape(t, 36), poses, betas, poses_root=root, mask=mask, slab=slab)
        assert all(torch.equal(x, y) for x, y in zip(got, want)), slab
    assert torch.isfinite(want.dist[mask == 1]).all() and want.inside.dtype == torch.bool


# ---- 4. inside ------------------------------------------------------------------------------------------------------------
def test_inside_matches_the_analytic_answer_on_convex_meshes_and_the_torus():
    margin = 2e-4                                                                        # >= 1e-4 m from the surface
    for name, (v, f) in (('cube', R.cube()), ('octahedron', R.octahedron()), ('icosahedron', R.icosahedron(1))):
        points = np.concatenate([R.displaced_from_faces(v, f, 96, margin, 51), R.displaced_from_faces(v, f, 96, -margin, 52),
                                 R.random_queries(64, 53, scale=1.2)])
        want = R.convex_inside(v, f, points)
        assert want[96:192].all() and not want[:96].any()
        got = query(v[None], f, points[None])
        assert np.array_equal(got.inside[0], want), name
        assert np.abs(got.dist[0, :192] - margin).max() < 2e-6, name                    # and they are that far from it
    nu, nv, delta = 24, 48, 0.02
    v, f = R.torus(nu, nv)
    assert R.torus_faceting_error(nu, nv) + 1e-4 < delta
    points = np.concatenate([R.torus_displaced(256, delta, 54), R.torus_displaced(256, -delta, 55)])
    got = query(v[None], f, points[None])
    assert np.array_equal(got.inside[0], R.torus_signed_distance(points) < 0)
    assert not got.inside[0, :256].any() and got.inside[0, 256:].all()
    assert (np.abs(got.dist[0] - delta) < R.torus_faceting_error(nu, nv) + 1e-6).all()


def test_grazing_rays_of_the_cube_are_exact():
    v, f = R.cube()
    points, want = R.grazing_rays()
    assert np.array_equal(query(v[None], f, points[None]).inside[0], want)
    assert np.array_equal(query(v[None], np.roll(f[::-1], 1, axis=1), points[None]).inside[0], want)


# ---- 5. the layers above the kernel -----------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def batch():
    """Two windows of five frames of the small model with 12 readings near the ground-truth surface, a mask with holes and
    a second window that ends after three frames; the estimate is the ground truth nudged."""
    smpl = SMPLLayer(H.small_model()).to(DEV)
    rng = np.random.default_rng(61)
    n, f, m = 2, 5, 12
    pose, root = rng.normal(0, 0.3, size=(n, f, 63)), rng.normal(0, 0.2, size=(n, f, 3))
    shape = rng.normal(0, 1.0, size=(n, 10))
    b = dict(pose=gpu(pose), root=gpu(root), shape=gpu(shape), pose_hat=gpu(pose + rng.normal(0, 0.05, size=pose.shape)),
             root_hat=gpu(root + rng.normal(0, 0.02, size=root.shape)), shape_hat=gpu(shape + 0.3),
             seq_lengths=torch.tensor([5, 3], device=DEV))
    flat = lambda x: x.reshape(n * f, -1)
    rep = lambda s: s.unsqueeze(1).expand(n, f, 10).reshape(n * f, 10)
    b['verts'] = smpl(poses_body=flat(b['pose']), betas=rep(b['shape']), poses_root=flat(b['root']))[0]
    b['verts_hat'] = smpl(poses_body=flat(b['pose_hat']), betas=rep(b['shape_hat']), poses_root=flat(b['root_hat']))[0]
    sites = rng.choice(smpl.n_vertices, size=m, replace=False)
    b['pos'] = (b['verts'][:, sites] + gpu(rng.normal(0, 0.01, size=(n * f, m, 3)))).reshape(n, f, m * 3)
    masks = (rng.uniform(size=(n, f, m)) > 0.25).astype(np.float32)
    masks[0, 1] = 0.0                                                                  # a frame without a reading
    b['masks'] = gpu(masks)
    return smpl, b


def engine_on(smpl, b, rows=slice(None)):
    e = SM.SkinDistanceEngine(smpl)
    e.compute(b['pose'][rows], b['shape'][rows], b['pose_hat'][rows], b['shape_hat'][rows], b['seq_lengths'][rows],
              b['root'][rows], b['root_hat'][rows], frame_mask=b['masks'][rows], marker_pos=b['pos'][rows],
              marker_masks=b['masks'][rows])
    return e


def test_engine_columns_match_the_restatement(batch):
    smpl, b = batch
    faces = np.asarray(H.small_model()['f'])
    n, f, m = 2, 5, 12
    pos = b['pos'].reshape(n * f, m, 3).cpu().numpy()
    count = b['masks'].cpu().numpy().reshape(n * f, m) == 1
    count[f + 3:] = False                                                              # the second window ends after 3 frames
    total = dict(n=0, d_hat=0.0, n_in=0, depth=0.0, d_gt=0.0, n_in_gt=0)
    for k in range(n * f):
        on = count[k]
        for key, verts in (('hat', b['verts_hat']), ('gt', b['verts'])):
            v = verts[k].cpu().numpy()
            dist = R.closest_point(v, faces, pos[k])['dist'][on]
            ins = R.inside(v, faces, pos[k])[on]
            if key == 'hat':
                total['n'] += int(on.sum()); total['d_hat'] += dist.sum(); total['n_in'] += int(ins.sum())
                total['depth'] += dist[ins].sum()
            else:
                total['d_gt'] += dist.sum(); total['n_in_gt'] += int(ins.sum())
    got = engine_on(smpl, b).get_metrics()
    print(got, total)
    assert total['n'] > 40 and got['Inside [%]'] == 100.0 * total['n_in'] / total['n']
    assert got['Inside GT [%]'] == 100.0 * total['n_in_gt'] / total['n']
    tol_mm = 1e3 * R.TOL_M                                                             # a mean of errors within TOL_M
    assert abs(got['Skin dist [mm]'] - 1e3 * total['d_hat'] / total['n']) <= tol_mm
    assert abs(got['Skin dist GT [mm]'] - 1e3 * total['d_gt'] / total['n']) <= tol_mm
    want_depth = 1e3 * total['depth'] / total['n_in'] if total['n_in'] else 0.0
    assert abs(got['Depth [mm]'] - want_depth) <= tol_mm
    assert got['Skin dist GT [mm]'] < got['Skin dist [mm]']                            # the readings were made on the truth


def test_engine_merge_of_two_halves_equals_the_whole(batch):
    smpl, b = batch
    whole = engine_on(smpl, b)
    first, second = engine_on(smpl, b, slice(0, 1)), engine_on(smpl, b, slice(1, 2))
    first.merge(second.state())
    assert np.array_equal(first.state()['sums'], whole.state()['sums'])
    assert first.get_metrics() == whole.get_metrics()
    assert whole.state()['sums'].shape == (4 + 3, 6)                                   # frames with a reading that count


def test_evaluate_with_a_skin_engine_changes_nothing_else():
    from em_pose_amd.data.data import AMASSBatch, AMASSSample
    from em_pose_amd.data.transforms import ToTensor, get_end_to_end_preprocess_fn
    from em_pose_amd.eval.helpers import evaluate
    from em_pose_amd.eval.metrics import MetricsEngine
    from em_pose_amd.helpers.configuration import lgd_config
    from em_pose_amd.nn.models import create_model
    case = H.load_case('train_lgdrnn12_n2')
    meta = case['meta']
    model, vids = H.small_model(), [int(v) for v in meta['vertex_ids']]
    smpl = SMPLLayer(model).to(DEV)
    cfg = lgd_config(int(meta['n_markers']), bool(meta['rnn']), int(meta['N']), hidden=32, rnn_hidden=32)
    net = create_model(cfg, SMPLLayer(model))
    net.load_state_dict(H.sd_to_torch(case['sd']), strict=False)
    net.vertex_ids = vids
    net = net.to(DEV).eval()
    rng = np.random.default_rng(9)
    offsets = {'means': rng.normal(0, 0.02, size=(12, 3)).astype(np.float32), 'covs': None,
               'r': np.tile(np.eye(3, dtype=np.float32), (12, 1, 1)), 'vertex_ids': np.asarray(vids)}
    fn = get_end_to_end_preprocess_fn(cfg, smpl, [offsets])
    batches = ((6, 4), (5,))

    def loader():
        r = np.random.default_rng(10)
        for lens in batches:
            yield AMASSBatch.from_sample_list([ToTensor()(AMASSSample(
                's', r.normal(0, 0.2, size=(n, 66)).astype(np.float32), r.normal(0, 1, size=10).astype(np.float32),
                np.zeros((n, 3), np.float32), 60.0)) for n in lens])
    plain, with_engine, se = MetricsEngine(smpl), MetricsEngine(smpl), SM.SkinDistanceEngine(smpl)
    se.merge({'sums': np.ones((3, 6))})                                                # `evaluate` resets the engine
    losses = evaluate(loader(), net, fn, plain, device=torch.device(DEV))
    losses_se = evaluate(loader(), net, fn, with_engine, device=torch.device(DEV), skin_engine=se)
    assert losses == losses_se and plain.get_metrics() == with_engine.get_metrics()
    rows = se.state()['sums']
    assert rows.shape == (6 + 4 + 5, 6) and (rows[:, 0] == 12).all()                   # every frame that counts, 12 readings
    got = se.get_metrics()
    print(got)
    # a reading sits at its vertex plus its offset, so it is no further from the ground-truth surface than the offset is long
    assert 0 < got['Skin dist GT [mm]'] <= 1e3 * np.linalg.norm(offsets['means'], axis=1).mean() + 1e-3
    assert got['Skin dist GT [mm]'] < got['Skin dist [mm]']
    assert 0 <= got['Inside [%]'] <= 100 and got['Depth [mm]'] >= 0


def test_compute_loss_and_metrics_prints_a_further_table_line(capsys):
    from em_pose_amd.data.data import AMASSBatch, AMASSSample
    from em_pose_amd.data.transforms import ToTensor, get_end_to_end_preprocess_fn
    from em_pose_amd.eval.helpers import compute_loss_and_metrics
    from em_pose_amd.helpers.configuration import lgd_config
    from em_pose_amd.nn.models import create_model
    case = H.load_case('train_lgdrnn12_n2')
    meta = case['meta']
    model, vids = H.small_model(), [int(v) for v in meta['vertex_ids']]
    smpl = SMPLLayer(model).to(DEV)
    cfg = lgd_config(int(meta['n_markers']), bool(meta['rnn']), int(meta['N']), hidden=32, rnn_hidden=32)
    net = create_model(cfg, SMPLLayer(model))
    net.load_state_dict(H.sd_to_torch(case['sd']), strict=False)
    net.vertex_ids = vids
    net = net.to(DEV).eval()
    offsets = {'means': np.full((12, 3), 0.01, np.float32), 'covs': None,
               'r': np.tile(np.eye(3, dtype=np.float32), (12, 1, 1)), 'vertex_ids': np.asarray(vids)}
    fn = get_end_to_end_preprocess_fn(cfg, smpl, [offsets])

    def loader():
        r = np.random.default_rng(10)
        yield AMASSBatch.from_sample_list([ToTensor()(AMASSSample(
            's', r.normal(0, 0.2, size=(n, 66)).astype(np.float32), r.normal(0, 1, size=10).astype(np.float32),
            np.zeros((n, 3), np.float32), 60.0)) for n in (5, 3)])
    plain = compute_loss_and_metrics(loader(), net, fn, 'm', smpl_model=smpl, device=torch.device(DEV))
    printed_plain = capsys.readouterr().out
    skin = compute_loss_and_metrics(loader(), net, fn, 'm', smpl_model=smpl, device=torch.device(DEV), skin_distance=True)
    printed_skin = capsys.readouterr().out
    assert plain == skin                                                               # the returned values are the same
    assert 'Skin dist' not in printed_plain and printed_skin.startswith(printed_plain)
    extra = printed_skin[len(printed_plain):].splitlines()
    assert len(extra) == 3 and all(c in extra[0] for c in SM.SkinDistanceEngine.COLUMNS)
    values = [float(x) for x in extra[2].split()[1:]]
    assert len(values) == 5 and all(np.isfinite(x) and x >= 0 for x in values)


def test_evaluate_real_script_prints_the_skin_table_to_stderr():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root + os.pathsep + os.environ.get('PYTHONPATH', ''))
    res = subprocess.run([sys.executable, os.path.join(root, 'scripts', 'evaluate_real.py'), '--synthetic',
                          '--max_sequences', '2', '--skin_distance'], env=env, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, timeout=600)
    out, err_text = res.stdout.decode(), res.stderr.decode()
    print(out)
    print(err_text)
    assert res.returncode == 0, err_text[-2000:]
    # stdout is what it is without the flag: the metric table and the throughput line, no word of the skin distance
    lines = out.splitlines()
    assert len(lines) == 6 and 'MPJPE [mm]' in lines[0] and 'Overall average' in lines[4] and 'frames/s' in lines[5]
    assert 'Skin dist' not in out and 'Inside' not in out and 'Depth' not in out
    err = err_text.splitlines()
    head = [ln for ln in err if 'Skin dist [mm]' in ln]
    assert len(head) == 1
    assert [head[0].index(c) for c in SM.SkinDistanceEngine.COLUMNS] == sorted(head[0].index(c)
                                                                             for c in SM.SkinDistanceEngine.COLUMNS)
    overall = [ln for ln in err if 'Overall average' in ln]
    assert len(overall) == 1
    values = [float(x) for x in overall[0].split('Overall average')[1].split()]
    assert len(values) == 5 and all(np.isfinite(x) and x >= 0 for x in values) and values[0] > 0 and values[1] > 0
    assert len([ln for ln in err if ln.strip().startswith(('0 ', '1 ')) and 'synthetic' in ln]) == 2   # a row per recording


def test_search_placement_reports_the_skin_distance():
    from em_pose_amd.data import placement as PL
    from em_pose_amd.data.offsets import pooled_recordings, root_normalized_poses
    from tests import offset_estimation_ref as REF
    from tests import placement_ref as PREF
    model, ids = H.small_model(), REF.small_ids()
    samples, _ = PREF.recordings(model, ids, [('x', (40, 25))], 71, offset_sd=0.01)
    smpl = SMPLLayer(model).to(DEV)
    found = PL.search_placement(smpl, samples, slab=16)['all']
    assert found['skin_mm'].shape == (12,) and found['skin_mm'].dtype == np.float32
    rec = pooled_recordings(smpl, samples, None, 12, False, DEV, 'test')
    poses = root_normalized_poses(smpl, rec, DEV)
    verts = smpl(poses_body=poses[:, 3:], betas=gpu(rec['betas']), poses_root=poses[:, :3])[0].cpu().numpy()
    faces = np.asarray(model['f'])
    dist = np.stack([R.closest_point(verts[k], faces, rec['pos'][k])['dist'] for k in range(verts.shape[0])])
    read = rec['masks'] == 1
    want = 1e3 * np.where(read, dist, 0.0).sum(axis=0) / read.sum(axis=0)
    assert np.array_equal(found['counts'], read.sum(axis=0))
    assert (np.abs(found['skin_mm'] - want) <= 1e3 * R.TOL_M + 1e-7 * want).all(), np.abs(found['skin_mm'] - want).max()
    assert (found['skin_mm'] <= found['rms_mm'] + 1e-3).all()                          # the surface is never further than a vertex
    other = PL.search_placement(smpl, samples, slab=64)['all']['skin_mm']              # (float64 sums in another order)
    assert np.allclose(other, found['skin_mm'], rtol=1e-6, atol=0)
