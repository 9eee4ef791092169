"""GPU tier: the cell-grid route of the fixed-radius search (sc_kernels_gno_grid.h) on an MI355X.  Every case calls
method="grid"; the yardstick is the brute-force route on the same device, byte for byte (both evaluate the same fp32
expression: no band, no excluded query), and on lattices the float64 helper (tests/gno_reference.py)."""
import numpy as np
import pytest
import torch

import gno_grid_cases as gc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _search():
    from neuraloperator_amd import engine
    return engine.radius_search


# ---------------------------------------------------------------------------------------------------------- 1. lattices
@pytest.mark.parametrize("d,L,r,n,m", gc.LATTICES)
def test_grid_on_a_lattice_is_exact_and_inclusive(d, L, r, n, m):
    gc.check_lattice(_search(), d, L, r, n, m, DEV)


# ------------------------------------------------------------------------------------------------------ 2. against brute
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("n,m", gc.SHAPES)
def test_grid_equals_brute_on_random_points(d, n, m):
    data, queries = gc.random_pair(d, n, m)
    if n > 3:
        queries[0] = data[3]                                 # a coincident pair
    got = gc.check_grid_equals_brute(_search(), data, queries, gc.RADII[d], DEV)
    assert n < 60 or got["neighbors_index"].numel() > 0


def test_sparse_rows_and_many_empty_cells():
    data, queries = gc.random_pair(3, 20000, 4097)
    got = gc.check_grid_equals_brute(_search(), data, queries, 0.01, DEV)
    deg = np.diff(got["neighbors_row_splits"].cpu().numpy())
    cell, G = gc.mirrored_cells(data.numpy(), 0.01)
    empty = int(np.prod(G)) - len(np.unique(cell))
    print(f"grid {G}: {empty} empty cells, {int((deg == 0).sum())} empty rows of {len(deg)}, {int(deg.sum())} edges")
    assert (deg == 0).mean() > 0.5 and deg.sum() > 0 and empty > 1000


@pytest.mark.parametrize("d", [1, 2, 3])
def test_degenerate_grid(d):
    data, queries, r = gc.box_edge_cases()[f"degenerate_grid_{d}d"]
    _, G = gc.mirrored_cells(data.numpy(), r)
    assert max(G) <= 2
    gc.check_grid_equals_brute(_search(), data, queries, r, DEV)


# -------------------------------------------------------------------------------------------- 3. long rows, full cells
def test_rows_past_the_staged_capacity_and_full_cells():
    gc.check_long_rows(_search(), 8192, 5000, 64, 0.1, DEV)


# ----------------------------------------------------------------------------------------------------------- 4. box edges
@pytest.mark.parametrize("name", [k for k in gc.box_edge_cases() if not k.startswith("degenerate")])
def test_box_edges(name):
    data, queries, r = gc.box_edge_cases()[name]
    got = gc.check_grid_equals_brute(_search(), data, queries, r, DEV)
    assert got["neighbors_index"].numel() > 0
    if name == "cell_cap_binds_1d":
        assert float(data.max() - data.min()) / r > gc.GRID_CAP[1]
    if name == "zero_radius":
        assert np.all(got["weights"].cpu().numpy() == np.float32(1e-14))


# ------------------------------------------------------------------------------------------------ 6. repeats, the layer
def test_two_calls_give_the_same_bytes():
    from neuraloperator_amd import NeighborSearch
    data, queries = (t.to(DEV) for t in gc.ball_case(8192, 5000, 64, 0.1, seed=8))
    a = _search()(data, queries, 0.1, True, method="grid")
    gc.assert_same_bytes(_search()(data, queries, 0.1, True, method="grid"), a)
    gc.assert_same_bytes(NeighborSearch(return_norm=True, method="grid")(data, queries, 0.1), a)


def test_layer_on_the_grid_equals_the_layer_on_brute():
    res = gc.layer_on_both_routes(DEV)
    assert len(res["grid"]) == len(res["brute"]) > 3
    for a, b in zip(res["grid"], res["brute"]):
        assert a.tobytes() == b.tobytes()
