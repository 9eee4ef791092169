"""CPU tier: the cell-grid route of the fixed-radius search (sc_kernels_gno_grid.h) in host emulation.  Every case calls
method="grid"; the yardstick is the brute-force route of the same emulation build, byte for byte (both evaluate the same
fp32 expression: no band, no excluded query), and on lattices the float64 helper (tests/gno_reference.py).  The two
largest shapes of the GPU tier -- (2049, 4097) and the sparse 20 000-point case -- are left to it: the emulated ballots
of the brute-force route take a minute there; (2049, 129) stands in for them here."""
import ctypes

import numpy as np
import pytest
import torch

import gno_grid_cases as gc
from emu_engine import engine_on_emulation
from neuraloperator_amd import NeighborSearch, _lib, engine


@pytest.fixture(scope="module")
def emu():
    with engine_on_emulation() as lib:
        yield lib


# ---------------------------------------------------------------------------------------------------------- 1. lattices
@pytest.mark.parametrize("d,L,r,n,m", gc.LATTICES)
def test_grid_on_a_lattice_is_exact_and_inclusive(emu, d, L, r, n, m):
    gc.check_lattice(engine.radius_search, d, L, r, n, m)


# ------------------------------------------------------------------------------------------------------ 2. against brute
@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("n,m", gc.SHAPES[:-1] + [(2049, 129)])
def test_grid_equals_brute_on_random_points(emu, d, n, m):
    data, queries = gc.random_pair(d, n, m)
    if n > 3 and m > 0:
        queries[0] = data[3]                                 # a coincident pair
    got = gc.check_grid_equals_brute(engine.radius_search, data, queries, gc.RADII[d])
    assert n < 60 or got["neighbors_index"].numel() > 0


@pytest.mark.parametrize("d", [1, 2, 3])
def test_degenerate_grid(emu, d):
    data, queries, r = gc.box_edge_cases()[f"degenerate_grid_{d}d"]
    _, G = gc.mirrored_cells(data.numpy(), r)
    assert max(G) <= 2
    gc.check_grid_equals_brute(engine.radius_search, data, queries, r)


# -------------------------------------------------------------------------------------------- 3. long rows, full cells
def test_rows_past_the_staged_capacity_and_full_cells(emu):
    """the smallest sizes that cross both constants: 160 points in the ball (> GRID_STAGE, > a wave)"""
    gc.check_long_rows(engine.radius_search, 400, 160, 24, 0.1)


# ----------------------------------------------------------------------------------------------------------- 4. box edges
@pytest.mark.parametrize("name", [k for k in gc.box_edge_cases() if not k.startswith("degenerate")])
def test_box_edges(emu, name):
    data, queries, r = gc.box_edge_cases()[name]
    got = gc.check_grid_equals_brute(engine.radius_search, data, queries, r)
    assert got["neighbors_index"].numel() > 0
    if name == "cell_cap_binds_1d":
        ext = float(data.max() - data.min())
        assert ext / r > gc.GRID_CAP[1]
    if name == "zero_radius":
        assert np.all(got["weights"].numpy() == np.float32(1e-14))


# --------------------------------------------------------------------------------------------------------- 5. non-finite
@pytest.mark.parametrize("d", [1, 2, 3])
def test_non_finite_coordinates(emu, d):
    data, queries = gc.random_pair(d, 300, 90)
    nan, inf = float("nan"), float("inf")
    for i, v in ((3, nan), (50, inf), (120, -inf), (299, nan)):
        data[i, i % d] = v
    bad_q = (0, 17, 40, 89)
    for i, v in zip(bad_q, (nan, inf, -inf, nan)):
        queries[i, (i + 1) % d] = v
    queries[5] = data[7]
    got = gc.check_grid_equals_brute(engine.radius_search, data, queries, 3 * gc.RADII[d])
    rs, idx = got["neighbors_row_splits"].numpy(), got["neighbors_index"].numpy()
    assert all(rs[q + 1] == rs[q] for q in bad_q), "a non-finite query has no neighbour"
    assert not set(idx.tolist()) & {3, 50, 120, 299}, "a non-finite data point is nobody's neighbour"
    assert len(idx) > 50
    # no finite data point at all
    data[:] = nan
    got = gc.check_grid_equals_brute(engine.radius_search, data, queries, 0.2)
    assert got["neighbors_index"].numel() == 0


# ------------------------------------------------------------------------------------------------ 6. repeats, the layer
def test_two_calls_give_the_same_bytes(emu):
    data, queries = gc.ball_case(400, 160, 24, 0.1, seed=8)
    a = engine.radius_search(data, queries, 0.1, True, method="grid")
    gc.assert_same_bytes(engine.radius_search(data, queries, 0.1, True, method="grid"), a)
    gc.assert_same_bytes(NeighborSearch(return_norm=True, method="grid")(data, queries, 0.1), a)


def test_layer_on_the_grid_equals_the_layer_on_brute(emu):
    res = gc.layer_on_both_routes("cpu")
    assert len(res["grid"]) == len(res["brute"]) > 3
    for a, b in zip(res["grid"], res["brute"]):
        assert a.tobytes() == b.tobytes()


# ----------------------------------------------------------------------------------------- 7. refusals and route choice
def test_refusals_before_any_launch(emu):
    L = emu.lib
    buf = torch.zeros(1 << 16, dtype=torch.int64)
    p, big = buf.data_ptr(), buf.numel() * 8
    R = _lib.ScEngineLib.radius_desc
    ok = R(2, 4, 4, 0.5)
    need = L.sc_radius_grid_workspace_bytes(ctypes.byref(ok))
    assert 0 < need <= big
    assert emu.radius_grid_workspace_bytes(R(2, 4, 5, 0.5)) == need + 4, "a function of the descriptor alone"
    for desc in (R(0, 4, 4, 0.5), R(4, 4, 4, 0.5), R(2, -1, 4, 0.5), R(2, 4, -1, 0.5), R(2, 4, 4, -1.0),
                 R(2, 4, 4, float("nan"))):
        assert L.sc_radius_grid_workspace_bytes(ctypes.byref(desc)) == 0
        assert L.sc_radius_grid_count(ctypes.byref(desc), p, p, p, p, p, big, None) != 0
        assert "sc_engine" in L.sc_last_error().decode()
        assert L.sc_radius_grid_fill(ctypes.byref(desc), p, p, p, 3, p, p, p, big, None) != 0
    assert L.sc_radius_grid_workspace_bytes(None) == 0
    assert L.sc_radius_grid_count(None, p, p, p, p, p, big, None) != 0
    for args in ((None, p, p, p, p, big), (p, None, p, p, p, big), (p, p, None, p, p, big), (p, p, p, None, p, big),
                 (p, p, p, p, None, big), (p, p, p, p, p, need - 1), (p, p, p, p, p, 0)):
        assert L.sc_radius_grid_count(ctypes.byref(ok), *args, None) != 0
    assert float(buf.abs().sum()) == 0.0, "nothing was launched"
    for args in ((p, p, p, -3, p, p, p, big), (p, p, p, 3, None, p, p, big), (p, p, p, 3, p, p, None, big),
                 (p, p, p, 3, p, p, p, need - 1), (p, p, None, 3, p, p, p, big)):
        assert L.sc_radius_grid_fill(ctypes.byref(ok), *args, None) != 0
    assert L.sc_radius_grid_fill(ctypes.byref(R(2, 4, 4, 0.5, True)), p, p, p, 3, p, None, p, big, None) != 0
    # valid empty problems: zero splits, no workspace needed
    for n, m in ((0, 4), (5, 0), (0, 0)):
        splits, deg = torch.ones(m + 1, dtype=torch.int64), torch.ones(max(m, 1), dtype=torch.int32)
        desc = R(3, n, m, 0.5)
        assert L.sc_radius_grid_count(ctypes.byref(desc), p if n else None, p if m else None, deg.data_ptr(),
                                      splits.data_ptr(), None, 0, None) == 0
        assert splits.tolist() == [0] * (m + 1)
        assert L.sc_radius_grid_fill(ctypes.byref(desc), p if n else None, p if m else None, splits.data_ptr(), 0, None,
                                     None, None, 0, None) == 0
        got = engine.radius_search(gc.points(1, n, 3), gc.points(2, m, 3), 0.5, True, method="grid")
        assert got["neighbors_index"].numel() == 0 and got["neighbors_row_splits"].tolist() == [0] * (m + 1)


def test_method_and_route_choice(emu):
    data, queries = gc.points(1, 9, 2), gc.points(2, 5, 2)
    with pytest.raises(ValueError):
        engine.radius_search(data, queries, 0.3, method="nonsense")
    with pytest.raises(ValueError):
        NeighborSearch(method="nonsense")
    gc.assert_same_bytes(engine.radius_search(data, queries, 0.3, True),
                         engine.radius_search(data, queries, 0.3, True, method="grid"))
    assert engine.radius_route(5000, 3000, 3) == "brute"
    assert engine.radius_route(100_000, 262_144, 3) == "grid"
    assert engine.radius_route(3000, 5000, 1) == "brute" and engine.radius_route(262_144, 100_000, 2) == "grid"
    # never below 2^25 pair tests: every shape the GPU tier ran before this route existed stays where it was
    assert all(engine.radius_route(n, m, d) == "brute" for d in (1, 2, 3) for n in (1, 4096, 1 << 20)
               for m in (1, 4096, 1 << 20) if n * m < 1 << 25)
    assert engine.RADIUS_GRID_MIN_PAIRS >= 1 << 25


def test_an_overflowing_squared_radius_keeps_every_pair(emu):
    """r * r = inf in fp32: d2 <= inf holds for every pair without a NaN, an infinite coordinate included"""
    data, queries = gc.points(3, 70, 2), gc.points(4, 9, 2)
    data[4, 0], queries[2, 1] = float("inf"), float("nan")
    got = gc.check_grid_equals_brute(engine.radius_search, data, queries, 1e30)
    assert got["neighbors_index"].numel() == 70 * 8
