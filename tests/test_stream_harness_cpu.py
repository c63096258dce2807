"""CPU: the pure parts of tests/_stream_harness.py - no GPU and no library: groups partitions the clips of a case, frames_of lists their
frames, and the StreamCall at the top of each of the three stream GPU files describes the outputs include/zedo_hip.h documents."""
import numpy as np
import pytest
import torch

import test_joint_accel_stream_gpu as accel
import test_joint_stream_gpu as hard
import test_joint_stream_marginal_gpu as soft
from _stream_harness import frames_of, groups
from _temporal_ref import clips


@pytest.mark.parametrize("N,L", [(70, 35), (12, 4), (130, 130), (9, 9), (1, 1), (12, 5), (30, 13), (6, 4), (7, 6)])
def test_groups_partition_the_clips(N, L):
    """L divides N, one clip, a shorter last clip: every clip of clips(N, L) once, in order, the streams of a group of one length."""
    seq = clips(N, L)
    got = [(a, a + Lc) for starts, Lc in groups(N, L) for a in starts]
    assert got == list(zip(seq[:-1], seq[1:]))
    assert sorted(f for starts, Lc in groups(N, L) for f in frames_of(starts, Lc).reshape(-1).tolist()) == list(range(N))
    assert len(groups(N, L)) == (2 if N % L and N > L else 1)
    assert groups(N, L)[0][1] == min(L, N)


def test_groups_by_hand():
    assert groups(70, 35) == [([0, 35], 35)] and groups(130, 130) == [([0], 130)] and groups(9, 9) == [([0], 9)]
    assert groups(12, 5) == [([0, 5], 5), ([10], 2)] and groups(3, 5) == [([0], 3)]


def test_frames_of():
    f = frames_of([0, 5], 3)
    assert isinstance(f, np.ndarray) and f.tolist() == [[0, 1, 2], [5, 6, 7]]
    assert frames_of([4], 1).tolist() == [[4]] and frames_of([], 3).size == 0


def test_the_output_specifications_are_the_headers():
    """At (S, rows, J, H) = (2, 3, 5, 7): d_path_h [S,F+lag,J] i32 and d_cost [S,F+lag,J] f64 of the two selections; d_mean [..,3], d_cov
    [..,6], d_hmax i32, d_wmax, d_logz and the optional d_w [..,H] of the fusion; the prefixes, weights and caps on H of the ABI."""
    i32, f64 = torch.int32, torch.float64
    two = (((2, 3, 5), i32), ((2, 3, 5), f64))
    assert tuple(hard.CALL.outputs(2, 3, 5, 7)) == two and tuple(accel.CALL.outputs(2, 3, 5, 7)) == two
    assert tuple(soft.CALL.outputs(2, 3, 5, 7)) == (((2, 3, 5, 3), f64), ((2, 3, 5, 6), f64), ((2, 3, 5), i32), ((2, 3, 5), f64), ((2, 3, 5), f64),
                                                    ((2, 3, 5, 7), f64))
    assert [(c.prefix, c.weights, c.index, c.max_h, c.optional) for c in (hard.CALL, soft.CALL, accel.CALL)] == [
        ("zedo_joint_stream", ("lam",), 0, 1024, {}), ("zedo_joint_stream_marginal", ("lam", "tau"), 2, 1024, {"with_w": 5}),
        ("zedo_joint_accel_stream", ("lam_v", "lam_a"), 0, 64, {})]
    # the slots of [u, x, T, flush, state, outputs .., emit] that must not be NULL: all but T, flush and d_w
    assert hard.CALL.required() == accel.CALL.required() == (0, 1, 4, 5, 6, 7) and soft.CALL.required() == (0, 1, 4, 5, 6, 7, 8, 9, 11)
    assert all(c.outputs(2, 3, 5, 7)[c.index][1] == i32 for c in (hard.CALL, soft.CALL, accel.CALL))
