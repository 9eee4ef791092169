"""Inputs and checks the two tiers of the cell-grid radius search share (tests/test_emu_gno_grid.py,
tests/test_gpu_gno_grid.py): the cases of the grid route against the brute-force route, byte for byte.  numpy / torch on
the host; the caller moves the tensors to its device and passes `search` = engine.radius_search."""
import numpy as np
import torch

import gno_reference as gr

# constants of sc_kernels_gno_grid.h the shapes are cut from
GRID_LANES, GRID_STAGE, GRID_SCAN_BLOCK = 16, 128, 4096
GRID_MARGIN, GRID_SLACK = 2.0 ** -8, 2.0 ** -62
GRID_CAP = {1: 8192, 2: 1024, 3: 128}
WAVE = 64

RADII = {1: 0.004, 2: 0.05, 3: 0.12}
# chunk, wave and workgroup edges of both routes; the last one takes the row-split scan through a carry
SHAPES = [(1, 1), (63, 7), (65, 9), (1025, 33), (2049, 4097)]
# (d, L, r, n, m): pairs at distance exactly r whose two points lie in neighbouring cells
LATTICES = [(1, 4096, 8 / 4096, 2048, 257), (2, 256, 5 / 256, 4096, 257), (3, 64, 3 / 64, 4096, 257)]


def points(seed, n, d):
    return torch.rand(n, d, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def lattice(d, L, n, m):
    """gr.lattice_points moved off the origin by float32(0.5): still exact"""
    data, queries = gr.lattice_points(np.random.default_rng(100 + d), n, m, d, L)
    return data - np.float32(0.5), queries - np.float32(0.5)


def random_pair(d, n, m):
    return points(10 * d + n, n, d), points(77 + d + m, m, d)


def ball_case(n, n_ball, m, r, seed=3):
    """d = 3: n_ball of the n points inside a ball of radius r / 4 around (0.55, 0.55, 0.55) -- for r = 0.1 inside one
    cell of the grid over the unit box -- and the rest uniform; m queries, every fourth one inside the ball"""
    g = torch.Generator().manual_seed(seed)
    data = torch.rand(n, 3, generator=g)
    v = torch.randn(n_ball, 3, generator=g)
    v = v / v.norm(dim=1, keepdim=True) * (r / 4) * torch.rand(n_ball, 1, generator=g) ** (1 / 3)
    data[torch.randperm(n, generator=g)[:n_ball]] = 0.55 + v
    queries = torch.rand(m, 3, generator=g)
    queries[::4] = 0.55 + (torch.rand(len(queries[::4]), 3, generator=g) - 0.5) * (r / 4)
    return data.float().contiguous(), queries.float().contiguous()


def mirrored_cells(data, r):
    """the cell of every data point as k_grid_params / gno_grid_cell compute it (fp32 steps in fp32): (cells, G)"""
    data = np.asarray(data, np.float32)
    n, d = data.shape
    h = (float(r) + GRID_SLACK) * (1 + GRID_MARGIN)
    lo, hi = data.min(0), data.max(0)
    ext = hi.astype(np.float64) - lo.astype(np.float64)
    G = [int(min(np.floor(e / h) + 1, GRID_CAP[d])) if e > 0 else 1 for e in ext]
    budget = min(max(-(-4 * n // GRID_SCAN_BLOCK) * GRID_SCAN_BLOCK, GRID_SCAN_BLOCK), GRID_CAP[d] ** d)
    while int(np.prod(G)) > budget:
        k = int(np.argmax(G))                                # the first of the longest axes
        G[k] = (G[k] + 1) // 2
    cell = np.zeros(n, np.int64)
    for k in range(d):
        inv = np.float32(1.0 / max(h, ext[k] / G[k])) if G[k] > 1 else np.float32(0)
        t = np.floor((data[:, k] - lo[k]) * inv)
        cell = cell * G[k] + np.clip(t, 0, G[k] - 1).astype(np.int64)
    return cell, G


def box_edge_cases():
    """name -> (data, queries, radius)"""
    out = {}
    for d in (1, 2, 3):
        out[f"queries_outside_{d}d"] = (points(5 + d, 500, d), points(9 + d, 300, d) * 3 - 1, 2.5 * RADII[d])
    data, queries = points(21, 700, 3), points(22, 200, 3)
    data[:, 2], queries[:, 2] = 0.25, 0.25 + 0.03 * (queries[:, 2] - 0.5)
    out["planar_data_3d"] = (data, queries, 0.08)
    data, queries = torch.full((200, 3), 0.3), points(23, 50, 3)
    queries[::5] = 0.3
    queries[1::5] = 0.3 + 0.01 * (queries[1::5] - 0.5)
    out["coincident_data"] = (data, queries, 0.02)
    out["one_data_point"] = (torch.tensor([[0.4, 0.6]]), torch.cat([points(24, 40, 2), torch.tensor([[0.4, 0.6]])]), 0.3)
    data, queries = points(25, 300, 2), points(26, 100, 2)
    queries[::3] = data[:34]
    data[100:110] = data[0]
    out["zero_radius"] = (data, queries, 0.0)
    data = points(27, 1500, 1) * 4096
    queries = torch.cat([data[:150] + 5e-5 * (points(28, 150, 1) - 0.5) * 4, data[300:350], points(29, 60, 1) * 4096])
    out["cell_cap_binds_1d"] = (data, queries, 1e-4)
    for d in (1, 2, 3):                                      # one or two cells per axis
        out[f"degenerate_grid_{d}d"] = (points(30 + d, 400, d), points(40 + d, 150, d), 0.6)
    return out


def assert_same_bytes(got, want, return_norm=True):
    """two neighbour dicts: the same keys, dtypes, shapes and bytes"""
    keys = ["neighbors_row_splits", "neighbors_index"] + (["weights"] if return_norm else [])
    assert sorted(got) == sorted(want) == sorted(keys)
    for k in keys:
        a, b = got[k].detach().cpu().numpy(), want[k].detach().cpu().numpy()
        assert a.dtype == b.dtype and a.shape == b.shape, (k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), f"{k} differs in {int((a != b).sum())} of {a.size} entries"
    assert got["neighbors_row_splits"].dtype == torch.int64 and got["neighbors_index"].dtype == torch.int64
    if return_norm:
        assert got["weights"].dtype == torch.float32


def check_grid_equals_brute(search, data, queries, radius, dev="cpu"):
    """both routes on the same tensors, with and without weights; returns the grid route's dict"""
    data, queries = data.to(dev), queries.to(dev)
    got = search(data, queries, radius, True, method="grid")
    assert_same_bytes(got, search(data, queries, radius, True, method="brute"))
    plain = search(data, queries, radius, False, method="grid")
    assert_same_bytes(plain, {k: v for k, v in got.items() if k != "weights"}, return_norm=False)
    return got


def check_lattice(search, d, L, r, n, m, dev="cpu"):
    """the grid route against the float64 helper, bit for bit: pairs at distance exactly r and coincident pairs"""
    data, queries = lattice(d, L, n, m)
    d2 = gr.squared_distances(data, queries)
    ref = gr.radius_search(data, queries, r, True)
    on_r, coincident = int((d2 == r * r).sum()), int((d2 == 0.0).sum())
    print(f"d={d}: {on_r} pairs at distance r, {coincident} coincident, {len(ref['neighbors_index'])} edges")
    assert on_r >= 100 and coincident >= 5
    rows, cols = np.nonzero(d2 <= r * r)
    np.testing.assert_array_equal(cols, ref["neighbors_index"])
    got = search(torch.from_numpy(data).to(dev), torch.from_numpy(queries).to(dev), r, True, method="grid")
    assert got["neighbors_index"].dtype == torch.int64 and got["neighbors_row_splits"].dtype == torch.int64
    assert got["weights"].dtype == torch.float32
    np.testing.assert_array_equal(got["neighbors_row_splits"].cpu().numpy(), ref["neighbors_row_splits"])
    np.testing.assert_array_equal(got["neighbors_index"].cpu().numpy(), ref["neighbors_index"])
    want = d2[rows, cols].astype(np.float32)
    assert np.all(want.astype(np.float64) == d2[rows, cols])                 # exactly representable
    want[want == 0] = np.float32(1e-14)
    w = got["weights"].cpu().numpy()
    assert np.array_equal(w.view(np.int32), want.view(np.int32)), "weights are float32(d2) bit for bit"


def check_long_rows(search, n, n_ball, m, r, dev="cpu"):
    """rows past the on-chip ordering capacity and a cell with more points than one pass of a wave"""
    data, queries = ball_case(n, n_ball, m, r)
    cell, G = mirrored_cells(data.numpy(), r)
    fullest = int(np.bincount(cell).max())
    got = check_grid_equals_brute(search, data, queries, r, dev)
    longest = int(np.diff(got["neighbors_row_splits"].cpu().numpy()).max())
    print(f"grid {G}: fullest cell {fullest} points, longest row {longest}")
    assert longest > GRID_STAGE and longest >= n_ball
    assert fullest > WAVE > GRID_LANES


def layer_on_both_routes(dev, name="3d_linear_halfcos"):
    """GNOBlock forward and backward with the search on "grid" and on "brute": (out, grads) of each"""
    from functools import partial
    from neuraloperator_amd import GNOBlock
    from neuraloperator_amd.gno import LinearChannelMLP
    cfg = gr.CASES[name]
    assert cfg["d"] == 3
    wfn = partial(gr.half_cos, radius=cfg["radius"] ** 2, scale=1.0) if cfg["weighting"] == "half_cos" else None
    torch.manual_seed(11)
    block = GNOBlock(**gr.block_kwargs(cfg, wfn, LinearChannelMLP)).to(dev)
    y, x, f = (None if t is None else t.to(dev) for t in gr.case_inputs(cfg, 4))
    res = {}
    for method in ("grid", "brute"):
        block.neighbor_search.method = method
        block.zero_grad(set_to_none=True)
        fin = f.clone().requires_grad_(True)
        out = block(y, x, fin)
        out.backward(torch.ones_like(out) * 0.5)
        res[method] = [out.detach().cpu().numpy(), fin.grad.cpu().numpy()] + \
            [p.grad.cpu().numpy() for p in block.parameters()]
    assert float(np.abs(res["grid"][0]).sum()) > 0
    return res
