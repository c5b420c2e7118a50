"""
nn/train_engine.py on side streams: every placement that `stream_plan` can produce -- all 16 subsets of
LgdTrainEngine.side_parts with `two_streams` on, and per-application weight gradients (`batched_wgrad` off) with none and
all of them -- runs the same kernels in the same order per accumulator as the single-stream step: losses, outputs, every
parameter gradient and every BatchNorm running statistic are bit-identical to it.

The construction is the one of test_hip_round4.py::test_training_step_on_side_streams_equals_the_single_stream_step:
64 windows x 32 frames = 2048 rows at hidden width 64, the smallest shape that takes the side streams without lowering
`two_streams_min_frames`, the x3 weight packing (>= 1024 rows, width on the 64 grid) and the epilogue-statistics route at
once.  `batched_wgrad` off adds the update networks' gradients in another order than the batched product, so those two
runs are held to the single-stream step with `batched_wgrad` off (and, for what no weight gradient enters -- losses,
outputs, running statistics -- to the batched one as well).
"""
import itertools

import numpy as np
import pytest
import torch

from oracle import torch_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PARTS = ('fwd', 'bwd', 'bwd3', 'wgrad')
SUBSETS = [tuple(p for p, on in zip(PARTS, bits) if on) for bits in itertools.product((False, True), repeat=4)]
B, F = 64, 32


@pytest.fixture(scope='module')
def scene():
    """Body model, twelve sensor vertices, one batch of synthetic windows and its ground-truth joints: shared, read-only."""
    from em_pose_amd import synthetic
    from tests import helpers as H
    model = H.small_model()
    bm = R.BodyModelTensors(model)
    vids = [int(v) for v in np.random.default_rng(5).choice(model['v_template'].shape[0], 12, replace=False)]
    tables = R.sensor_tables(model['f'], vids)

    def sensors(poses, betas, o_r, o_t):
        with torch.no_grad():
            p, o, _ = R.estimated_markers(bm, tables, vids, torch.from_numpy(poses), torch.from_numpy(betas),
                                          torch.from_numpy(o_r), torch.from_numpy(o_t))
        return p.numpy(), o.numpy()
    w = synthetic.make_windows(B, F, 3, sensors)
    with torch.no_grad():
        _, _, jgt = R.estimated_markers(bm, tables, vids, torch.from_numpy(w['poses'].reshape(-1, 66)),
                                        torch.from_numpy(np.repeat(w['shapes'], F, axis=0)),
                                        torch.from_numpy(np.repeat(w['offset_r'], F, axis=0)),
                                        torch.from_numpy(np.repeat(w['offset_t'], F, axis=0)))
    return model, vids, w, jgt.reshape(B, F, -1).float()


@pytest.mark.parametrize('rnn', [True, False], ids=['lgd_rnn', 'lgd'])
def test_every_stream_placement_equals_the_single_stream_step(scene, rnn):
    from em_pose_amd.bodymodels.smpl import SMPLLayer
    from em_pose_amd.data.data import SyntheticBatch
    from em_pose_amd.helpers.configuration import lgd_config
    from em_pose_amd.nn.models import create_model
    from em_pose_amd.nn.train_engine import LgdTrainEngine
    model, vids, w, jgt = scene
    torch.manual_seed(7)
    net = create_model(lgd_config(12, rnn, 2, hidden=64, rnn_hidden=64), SMPLLayer(model))
    net.vertex_ids = vids
    net = net.to(DEV).train()
    state0 = {k: v.clone() for k, v in net.state_dict().items()}
    lens = torch.full((B,), F, dtype=torch.int64, device=DEV)
    lens[3] = 17

    def step(two, parts, batched):
        LgdTrainEngine.two_streams, LgdTrainEngine.side_parts, LgdTrainEngine.batched_wgrad = two, parts, batched
        net.load_state_dict(state0)
        batch = SyntheticBatch(w, lens, device=DEV)
        batch.joints_gt = jgt.to(DEV)
        net.zero_grad()
        out = net(batch)
        assert net._engine is not None and net._engine._use_side == two
        total, vals = net.backward(batch, out)
        torch.cuda.synchronize()
        return {'losses': vals,
                'out': {k: v.detach().clone() for k, v in out.items()},
                'grads': {k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None},
                'stats': {k: v.clone() for k, v in net.state_dict().items() if 'running' in k}}

    def same(got, want, what, groups=('losses', 'out', 'grads', 'stats')):
        for group in groups:
            assert got[group].keys() == want[group].keys(), (what, group)
            for k, v in want[group].items():
                equal = torch.equal(got[group][k], v) if torch.is_tensor(v) else got[group][k] == v
                assert equal, (what, group, k)

    saved = LgdTrainEngine.two_streams, LgdTrainEngine.side_parts, LgdTrainEngine.batched_wgrad
    try:
        single = step(False, PARTS, True)
        assert len(single['out']) >= 3 and len(single['grads']) > 20 and len(single['stats']) > 0
        for parts in SUBSETS:
            same(step(True, parts, True), single, parts)
        single_per_application = step(False, PARTS, False)
        same(single_per_application, single, 'per application', groups=('losses', 'out', 'stats'))
        for parts in ((), PARTS):
            got = step(True, parts, False)
            same(got, single_per_application, ('per application', parts))
            same(got, single, ('per application', parts), groups=('losses', 'out', 'stats'))
    finally:
        LgdTrainEngine.two_streams, LgdTrainEngine.side_parts, LgdTrainEngine.batched_wgrad = saved
