"""
The stream plan of the hand-written training step (nn/train_engine.py, `stream_plan`): all 64 inputs -- `use_side` x the 16
subsets of LgdTrainEngine.side_parts x `deferred` -- against a table written out here by reading the placement rules (they
were read off the engine's forward / backward before the plan existed), not computed from the engine.  No GPU.
"""
import itertools

import pytest

from em_pose_amd.nn.train_engine import MAIN, LgdTrainEngine, StreamPlan, stream_plan

PARTS = ('fwd', 'bwd', 'bwd3', 'wgrad')
SUBSETS = [tuple(p for p, on in zip(PARTS, bits) if on) for bits in itertools.product((False, True), repeat=4)]
M = MAIN
# side streams in use and the weight gradients deferred: what 'bwd' / 'bwd3' / 'wgrad' select ('fwd' only sets fwd_split)
#   (bwd_split, pose_bwd, shape_bwd, pose_wgrad, shape_wgrad, join_before_wgrad, fork_before_wgrad)
REVERSE = {
    frozenset():                           (False, M, M, M, M, True, False),    # join (nothing is forked), products on main
    frozenset(['bwd3']):                   (False, M, M, M, M, True, False),    # 'bwd3' without 'bwd': no effect
    frozenset(['bwd']):                    (True, M, 0, M, M, True, False),     # shape net trails on side 0; join; main
    frozenset(['bwd', 'bwd3']):            (True, 1, 0, M, M, True, False),     # pose net on side 1 too; join both; main
    frozenset(['wgrad']):                  (False, M, M, 0, 0, False, True),    # fork side 0, both products there
    frozenset(['bwd3', 'wgrad']):          (False, M, M, 0, 0, False, True),    # 'bwd3' without 'bwd': no effect
    frozenset(['bwd', 'wgrad']):           (True, M, 0, 0, 0, False, True),     # pose backward ran on main: fork side 0 again
    frozenset(['bwd', 'bwd3', 'wgrad']):   (True, 1, 0, 1, 0, False, False),    # each behind its own backward: no fork
}
ALL_MAIN = (False, M, M, M, M, False, False)


def expected(use_side, parts, deferred):
    if not use_side:
        return StreamPlan(False, *ALL_MAIN)
    reverse = REVERSE[frozenset(parts) - {'fwd'}] if deferred else ALL_MAIN
    return StreamPlan('fwd' in parts, *reverse)


def test_the_table_covers_the_eight_reverse_sweep_choices():
    assert len(SUBSETS) == 16 and len(set(SUBSETS)) == 16
    assert set(REVERSE) == {frozenset(s) - {'fwd'} for s in SUBSETS} and len(REVERSE) == 8
    assert tuple(LgdTrainEngine.side_parts) == PARTS


@pytest.mark.parametrize('deferred', [True, False])
@pytest.mark.parametrize('parts', SUBSETS, ids=lambda s: '+'.join(s) or 'none')
@pytest.mark.parametrize('use_side', [True, False])
def test_stream_plan_equals_the_written_out_table(use_side, parts, deferred):
    assert stream_plan(use_side, parts, deferred) == expected(use_side, parts, deferred)


def test_without_side_streams_everything_is_on_main_with_no_fork_and_no_join():
    plans = [stream_plan(False, parts, deferred) for parts in SUBSETS for deferred in (True, False)]
    assert len(plans) == 32
    for plan in plans:
        assert plan == StreamPlan(fwd_split=False, bwd_split=False, pose_bwd=MAIN, shape_bwd=MAIN, pose_wgrad=MAIN,
                                  shape_wgrad=MAIN, join_before_wgrad=False, fork_before_wgrad=False)


def test_bwd3_without_bwd_changes_nothing():
    for use_side, deferred in itertools.product((True, False), repeat=2):
        for parts in SUBSETS:
            if 'bwd3' in parts and 'bwd' not in parts:
                without = tuple(p for p in parts if p != 'bwd3')
                assert stream_plan(use_side, parts, deferred) == stream_plan(use_side, without, deferred)


def test_per_application_weight_gradients_keep_the_reverse_sweep_on_main():
    for use_side in (True, False):
        for parts in SUBSETS:
            plan = stream_plan(use_side, parts, False)
            assert not plan.bwd_split and not plan.join_before_wgrad and not plan.fork_before_wgrad
            assert (plan.pose_bwd, plan.shape_bwd, plan.pose_wgrad, plan.shape_wgrad) == (MAIN,) * 4
            assert plan.fwd_split == (use_side and 'fwd' in parts)     # (the forward is joined every iteration)


def test_a_side_stream_is_used_only_where_it_was_forked():
    """Side 1 only ever follows a per-iteration fork of the pose network's backward; side 0 carries weight gradients either
    behind the shape network's backward (forked there) or after a fork of its own; and the products run on main only
    after the joins."""
    for parts in SUBSETS:
        plan = stream_plan(True, parts, True)
        if plan.pose_wgrad == 1:
            assert plan.pose_bwd == 1 and plan.shape_wgrad == 0 and plan.shape_bwd == 0 and not plan.fork_before_wgrad
        if plan.shape_wgrad == 0 and plan.pose_wgrad == 0:
            assert plan.fork_before_wgrad
        if plan.pose_wgrad is MAIN:
            assert plan.shape_wgrad is MAIN and plan.join_before_wgrad
        assert not (plan.join_before_wgrad and plan.fork_before_wgrad)
        assert plan.shape_bwd == (0 if plan.bwd_split else MAIN) and (plan.pose_bwd is MAIN or plan.bwd_split)
