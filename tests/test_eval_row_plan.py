"""The row plan of the batched evaluation driver (eval/helpers.py::plan_rows): which rows a chunk holds and where every
frame's metric row goes.  Host arithmetic on lengths and masks: no device, no model."""
import numpy as np
import pytest

from em_pose_amd.eval.helpers import plan_rows

WINDOW = 256


def _streaming_case():
    """The lengths of tests/test_hip_parity.py::_streaming_recordings, 1 % of the frames missing."""
    rng = np.random.default_rng(20231)
    lengths = [300, 700, 256, 40]
    return lengths, [rng.random(n) >= 0.01 for n in lengths]


def _edge_case():
    """Two equal lengths, a recording shorter than a window, a recording without a single valid frame."""
    rng = np.random.default_rng(7)
    lengths = [513, 100, 513, 260]
    valid = [rng.random(n) >= 0.05 for n in lengths]
    valid[3][:] = False
    return lengths, valid


CASES = {'streaming_recordings': _streaming_case, 'equal_short_and_empty': _edge_case}


@pytest.fixture(params=sorted(CASES))
def case(request):
    lengths, valid = CASES[request.param]()
    return lengths, valid, plan_rows(lengths, valid, WINDOW)


def test_rows_with_frames_are_a_prefix_of_the_order(case):
    lengths, _, plan = case
    assert sorted(plan.order) == list(range(len(lengths)))
    assert [lengths[i] for i in plan.order] == sorted(lengths, reverse=True) == list(plan.lengths)
    assert len(plan.chunks) == (max(lengths) + WINDOW - 1) // WINDOW
    for c, ch in enumerate(plan.chunks):
        assert ch.sf == c * WINDOW
        with_frames = [lengths[i] > ch.sf for i in plan.order]
        assert with_frames == [True] * ch.k + [False] * (len(lengths) - ch.k)
        assert list(ch.lens) == [min(WINDOW, lengths[i] - ch.sf) for i in plan.order[:ch.k]]
        assert ch.f == ch.lens[0]
        assert list(plan.lens[c]) == list(ch.lens) + [0] * (len(lengths) - ch.k)


def test_base_is_in_recording_order(case):
    lengths, valid, plan = case
    assert plan.base[0] == 0 and plan.total == plan.base[-1] == sum(int(v.sum()) for v in valid)
    assert list(np.diff(plan.base)) == [int(v.sum()) for v in valid]


def test_dest_is_a_permutation_and_invalid_frames_go_to_the_spare_row(case):
    lengths, valid, plan = case
    assert plan.valid.shape == plan.dest.shape == (len(lengths), max(lengths))
    for j, i in enumerate(plan.order):
        assert np.array_equal(plan.valid[j, :lengths[i]], valid[i]) and not plan.valid[j, lengths[i]:].any()
    assert sorted(plan.dest[plan.valid].tolist()) == list(range(plan.total))
    assert (plan.dest[~plan.valid] == plan.total).all()


def test_dest_follows_the_frames_of_a_recording(case):
    lengths, valid, plan = case
    for j, i in enumerate(plan.order):
        d = plan.dest[j][plan.valid[j]]
        assert d.tolist() == list(range(plan.base[i], plan.base[i + 1]))


def test_every_recording_ends_once_in_the_chunk_of_its_last_frame(case):
    lengths, _, plan = case
    ended = [(i, c) for c, ch in enumerate(plan.chunks) for i in ch.ended]
    assert sorted(ended) == [(i, (n - 1) // WINDOW) for i, n in enumerate(lengths) if n > 0]


def test_a_recording_without_a_valid_frame_owns_no_rows():
    lengths, valid, = _edge_case()
    plan = plan_rows(lengths, valid, WINDOW)
    assert plan.base[3] == plan.base[4]
    assert 3 in plan.chunks[1].ended
    assert (plan.dest[plan.order.index(3)] == plan.total).all()
