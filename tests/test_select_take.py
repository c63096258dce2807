"""CPU: take_rows - the winning row of every pose out of the gathered h-major rows (plain torch indexing, no kernel), and the
name of the file run.inference --select reproj writes."""
import pytest
import torch


def test_take_rows_picks_row_idx_times_n_plus_n():
    from zedo_hip.pipeline import take_rows
    H, N = 4, 3
    rows = torch.arange(H * N * 2, dtype=torch.float32).reshape(H * N, 2)
    idx = torch.tensor([3, 0, 2], dtype=torch.int32)
    assert torch.equal(take_rows(rows, idx, H, N), rows[[3 * N + 0, 0 * N + 1, 2 * N + 2]])
    assert take_rows(rows.reshape(H * N, 2, 1), idx, H, N).shape == (N, 2, 1)
    for bad in ([3, -1, 2], [3, 4, 2]):                      # a pose without a selected hypothesis / an index outside 0 .. H-1
        with pytest.raises(ValueError):
            take_rows(rows, torch.tensor(bad, dtype=torch.int32), H, N)
    with pytest.raises(ValueError):
        take_rows(rows[:-1], idx, H, N)


def test_selected_path_and_the_parser_switch():
    from run._driver import build_parser, selected_path
    assert selected_path("out/results.npy") == "out/results_selected.npz" and selected_path("res") == "res_selected.npz"
    for inference in (False, True):
        p = build_parser("x", inference=inference)
        assert p.parse_args(["--config", "c"]).select == "none" and p.parse_args(["--config", "c", "--select", "reproj"]).select == "reproj"
