"""CPU: the numpy reference of the hypothesis pruning (tests/_prune_ref.py) against the enumeration "sort all slots with a Python comparator
that states the contract's three clauses", and the plan parser of Pipeline.run_pruned / --prune."""
import numpy as np
import pytest

from _prune_ref import brute_order, case, gather_ref, keep_ref, order_ref


@pytest.mark.parametrize("H,N", [(1, 3), (2, 9), (3, 7), (7, 20), (13, 11), (50, 8)])
def test_the_lexsort_order_is_the_comparator_order(H, N):
    for seed in range(3):
        e = case(H, N, seed)
        o = order_ref(e, N)
        assert np.array_equal(o, brute_order(e, N))
        assert np.array_equal(np.sort(o, axis=0), np.broadcast_to(np.arange(H)[:, None], (H, N)))       # a permutation per pose
        for K in range(1, H + 1):
            k = keep_ref(e, N, K)
            assert k.shape == (K, N) and k.dtype == np.int32 and (np.diff(k, axis=0) > 0).all()
            assert all(set(k[:, n]) == set(o[:K, n]) for n in range(N))
        assert np.array_equal(keep_ref(e, N, H), np.broadcast_to(np.arange(H, dtype=np.int32)[:, None], (H, N)))


def test_the_order_on_a_case_written_out():
    nan, inf = np.nan, np.inf
    e = np.array([nan, 2.0, 0.0, inf, -0.0, 2.0, nan, 1.0])          # one pose, eight slots
    assert order_ref(e, 1)[:, 0].tolist() == [2, 4, 7, 1, 5, 3, 0, 6]
    assert keep_ref(e, 1, 3)[:, 0].tolist() == [2, 4, 7] and keep_ref(e, 1, 5)[:, 0].tolist() == [1, 2, 4, 5, 7]
    assert keep_ref(e, 1, 7)[:, 0].tolist() == [0, 1, 2, 3, 4, 5, 7]                                   # the higher NaN goes first


def test_the_gather_reference():
    H, N, J = 4, 3, 2
    x = np.arange(H * N * J * 3, dtype=np.float32).reshape(H * N, J, 3)
    T = -np.arange(H * N * 3, dtype=np.float32).reshape(H * N, 3)
    keep = np.array([[0, 1, 2], [3, -1, 4]], np.int32)
    xo, To, ho = gather_ref(keep, x, T)
    assert np.array_equal(xo[0], x[0]) and np.array_equal(xo[1], x[1 * N + 1]) and np.array_equal(xo[3], x[3 * N])
    assert np.isnan(xo[4]).all() and np.isnan(To[4]).all() and np.isnan(xo[5]).all()
    assert ho.tolist() == [[0, 1, 2], [3, -1, -1]] and np.array_equal(To[2], T[2 * N + 2])
    hyp = 10 + np.arange(H * N, dtype=np.int32).reshape(H, N)
    assert gather_ref(keep, x, T, hyp)[2].tolist() == [[10, 14, 18], [19, -1, -1]]


def test_parse_prune_plan_accepts_the_plans_of_the_documents():
    from zedo_hip.pipeline import parse_prune_plan, prune_row_steps
    assert parse_prune_plan("100:10", 50, 1000) == [(100, 10)]
    assert parse_prune_plan("0:25,200:5", 50, 1000) == [(0, 25), (200, 5)]
    assert parse_prune_plan(" 7:4 , 8:2 ", 6, 40) == [(7, 4), (8, 2)]
    assert parse_prune_plan("0:50", 50, 1000) == [(0, 50)] and parse_prune_plan("999:1", 50, 1000) == [(999, 1)]
    assert prune_row_steps([(100, 10)], 50, 1000) == (14000, 50000)                                     # 50*100 + 10*900
    assert prune_row_steps([(0, 50)], 50, 1000) == (50000, 50000) and prune_row_steps([], 50, 1000) == (50000, 50000)
    assert prune_row_steps([(0, 25), (200, 5)], 50, 1000) == (25 * 200 + 5 * 800, 50000)


@pytest.mark.parametrize("text,item", [("200:10,100:5", "100:5"),        # a descending step
                                       ("100:10,100:5", "100:5"),        # ... or a repeated one
                                       ("100:10,200:10", "200:10"),      # a keep that is not descending
                                       ("100:10,200:20", "200:20"),
                                       ("100:0", "100:0"),               # keep 0
                                       ("100:51", "100:51"),             # keep > H
                                       ("1000:10", "1000:10"),           # step >= S
                                       ("0:25,1000:5", "1000:5"),
                                       ("junk", "junk"), ("100", "100"), ("100:10:3", "100:10:3"), ("-1:3", "-1:3"), ("1.5:3", "1.5:3"),
                                       ("100:10,", ""), ("", "")])
def test_parse_prune_plan_names_the_offending_item(text, item):
    from zedo_hip.pipeline import parse_prune_plan
    with pytest.raises(ValueError) as e:
        parse_prune_plan(text, 50, 1000)
    assert repr(item) in str(e.value)


def test_the_parser_switch_and_the_file_name():
    from run._driver import build_parser, pruned_path
    assert pruned_path("out/results.npy") == "out/results_pruned.npz" and pruned_path("res") == "res_pruned.npz"
    for inference in (False, True):
        p = build_parser("x", inference=inference)
        assert p.parse_args(["--config", "c"]).prune is None and p.parse_args(["--config", "c", "--prune", "100:10"]).prune == "100:10"
