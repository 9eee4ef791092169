"""The banded stencil and loss kernels (sc_kernels_stencil.h: sc_band_apply, sc_sobolev_sums, sc_lp_grad) in host
emulation through the C-ABI against a float64 numpy evaluation of their own formulas with random 7-band tables: row
lengths that are no multiple of the wave (1, 4, 5, 67, 130), many groups with tiny rows (33 x 4 x 5), more rows than one
tile, periodic and clamped axes, the fused difference source, the per-group scale and the identity term; the adjoint
identity of every finite-difference operator; the sums kernel with one and with several chunks per line and a point
count that is no multiple of the chunk; bit-identical repeats; every refused argument returning its error.  The runners
and float64 formulas are those of finite_diff_reference, shared with the GPU tier (tests/test_gpu_stencil_kernels.py);
the kernel-edge cases of that tier which the emulation finishes quickly (EMU_BAND_KERNEL_CASES, EMU_SUMS_KERNEL_CASES)
run here at the same two bars, rel-L2 and per element |err| <= gamma_N A."""
import numpy as np
import pytest
import torch

import finite_diff_reference as fdr
from emu_engine import engine_on_emulation
from engine_runner import rel_l2
from finite_diff_reference import random_tables as _random_tables, random_terms as _terms, run_band as _band, \
    want_band as _want_band, want_sums as _want_sums
from neuraloperator_amd import engine


# dims, periodic, groups, n_src, n_out, n_terms, empty output, fused difference, scale, out_major
BAND_CASES = [((1,), (True,), 1, 1, 1, 1, None, False, False, False),
              ((4,), (False,), 5, 2, 2, 4, None, True, True, True),
              ((5,), (True,), 33, 1, 3, 3, 1, False, False, False),
              ((67,), (False,), 3, 3, 1, 5, None, False, True, False),
              ((130,), (True,), 2, 1, 2, 4, None, True, False, True),
              ((4, 5), (False, True), 33, 2, 2, 6, None, True, True, False),
              ((70, 130), (True, False), 2, 1, 1, 4, None, False, False, False),
              ((3, 2), (True, True), 4, 3, 3, 9, 2, False, True, True),
              ((5, 6, 67), (True, False, True), 2, 2, 3, 8, None, True, False, False),
              ((4, 35, 4), (False, True, False), 3, 3, 3, 12, None, False, True, True),
              ((2, 1, 3), (True, True, True), 2, 1, 1, 6, None, False, False, False)]


@pytest.mark.parametrize("case", BAND_CASES, ids=["x".join(map(str, c[0])) + f"-g{c[2]}-s{c[3]}-o{c[4]}" for c in BAND_CASES])
def test_band_apply_matches_float64(case):
    dims, periodic, groups, n_src, n_out, n_terms, empty, fused, scaled, out_major = case
    rng = np.random.default_rng(sum(dims) * 100 + groups)
    n_tab = tuple(1 + d for d in range(len(dims)))
    tabs = _random_tables(rng, dims, periodic, n_tab)
    terms = _terms(rng, n_src, n_out, len(dims), n_tab, n_terms, empty)
    u = torch.from_numpy(rng.standard_normal((groups, n_src) + dims).astype(np.float32))
    u2 = torch.from_numpy(rng.standard_normal((groups, n_src) + dims).astype(np.float32)) if fused else None
    scale = torch.from_numpy(rng.standard_normal(groups).astype(np.float32)) if scaled else None
    mul = torch.tensor([1.5]) if scaled else None
    with engine_on_emulation() as lib:
        y = _band(lib, u, u2, tabs, periodic, terms, n_out, out_major, scale, mul)
        y2 = _band(lib, u, u2, tabs, periodic, terms, n_out, out_major, scale, mul)
    sc = np.ones(groups) if scale is None else scale.numpy().astype(np.float64) * 1.5
    want = _want_band(u.numpy(), None if u2 is None else u2.numpy(), tabs, periodic, terms, n_out, sc)
    assert not torch.isnan(y).any()                                     # every addressed element is overwritten
    assert rel_l2(y.numpy(), want) <= 2e-6
    assert torch.equal(y, y2)                                           # the same bits twice
    if empty is not None:
        assert torch.all(y[:, empty] == 0)


def test_output_stride_leaves_the_neighbours_alone():
    rng = np.random.default_rng(3)
    dims, periodic = (5, 7), (True, False)
    tabs = _random_tables(rng, dims, periodic, (1, 1))
    u = torch.from_numpy(rng.standard_normal((3, 1) + dims).astype(np.float32))
    y = torch.full((3, 2, 35 + 3), 7.0)                                 # gaps behind every output
    with engine_on_emulation() as lib:
        lib.band_apply(u.data_ptr(), 0, y.data_ptr(), dims=dims, periodic=periodic, groups=3, n_src=1, n_out=2,
                       terms=((0, 0, 1.0, 0, 0), (0, 1, 1.0, 1, 0)), tabs=[torch.from_numpy(t).data_ptr() for t in tabs],
                       n_tab=(1, 1), y_group_stride=76, y_out_stride=38)
    assert torch.all(y[:, :, 35:] == 7.0) and not torch.any(y[:, :, :35] == 7.0)


@pytest.mark.parametrize("name", sorted(fdr.CASES))
def test_adjoint_identity_of_every_operator(name):
    """<D u, g> = <u, D^T g> with D^T the transposed tables on the same kernel, for D1 and D2 of every axis"""
    grid, h, periodic = fdr.CASES[name]
    g = torch.Generator().manual_seed(11)
    u, w = torch.randn(3, 1, *grid, generator=g), torch.randn(3, 1, *grid, generator=g)
    with engine_on_emulation():
        tabs = engine.finite_diff_tables(u.device, grid, h, periodic)
        for axis in range(len(grid)):
            for row in (0, 1):
                du = engine._band_apply(u, None, tabs, ((0, 0, 1.0, axis, row),), 1, False)
                dtw = engine._band_apply(w, None, tabs, ((0, 0, 1.0, axis, tabs.adj[axis][row]),), 1, False)
                m = torch.as_tensor(fdr.dense_matrix(grid[axis], h[axis], row + 1, periodic[axis]))
                assert fdr.rel_l2(du, fdr.apply_matrix(m, u.double(), axis - len(grid))) <= 2e-6
                lhs, rhs = float((du.double() * w).sum()), float((u.double() * dtw).sum())
                assert abs(lhs - rhs) <= 1e-5 * (abs(lhs) + abs(rhs) + 1e-30), (axis, row)


# dims, periodic, lines, h1, p, relative, root, mean, chunks asked for
SUM_CASES = [((70, 130), (True, False), 1, True, 2, True, True, False, 0),      # several chunks (3 of 9 tiles each)
             ((70, 130), (True, False), 3, True, 2, False, True, True, 5),
             ((4, 5), (False, True), 33, True, 2, True, False, False, 0),       # one chunk per line
             ((5, 6, 67), (True, False, True), 2, True, 2, False, False, False, 4),
             ((131,), (True,), 2, True, 2, True, True, True, 2),
             ((5000,), (True,), 1, False, 1, True, True, False, 0),             # 5 units, 4 chunks of 2: ragged end
             ((5000,), (True,), 3, False, 2, False, True, True, 3),
             ((3, 1367), (True, True), 2, False, 3, True, True, False, 2),
             ((3, 1367), (True, True), 2, False, 3, False, False, False, 1),
             ((6, 7), (True, True), 300, False, 2, True, True, True, 0)]        # more lines than one pass of stage 2


@pytest.mark.parametrize("case", SUM_CASES, ids=["x".join(map(str, c[0])) + f"-l{c[2]}-{'h1' if c[3] else 'lp'}{c[4]}-c{c[8]}"
                                                 for c in SUM_CASES])
def test_sobolev_sums_and_lp_grad_match_float64(case):
    dims, periodic, lines, h1, p, relative, root, mean, chunks = case
    rng = np.random.default_rng(sum(dims) + lines)
    tabs = _random_tables(rng, dims, periodic, (1,) * len(dims))
    tt = [torch.from_numpy(t).contiguous() for t in tabs]
    x = torch.from_numpy(rng.standard_normal((lines,) + dims).astype(np.float32))
    y = torch.from_numpy(rng.standard_normal((lines,) + dims).astype(np.float32))
    konst, eps = 0.37, 1e-3
    with engine_on_emulation() as lib:
        desc = lib.sobolev_desc(dims=dims, periodic=periodic, lines=lines, h1=h1, p=p, relative=relative, take_root=root,
                                reduce_mean=mean, konst=konst, eps=eps, tabs=[t.data_ptr() for t in tt] if h1 else None,
                                chunks=chunks)
        nbytes = lib.sobolev_workspace_bytes(desc)
        n_chunks = nbytes // (8 * lines)
        runs = []
        for _ in range(2):
            ws = torch.full((nbytes // 4,), float("nan"))
            v, dv, loss = torch.empty(lines), torch.empty(lines), torch.empty(1)
            lib.sobolev_sums(desc, x.data_ptr(), y.data_ptr(), ws.data_ptr(), nbytes, v.data_ptr(), dv.data_ptr(),
                             loss.data_ptr())
            runs.append((ws, v, dv, loss))
        if not h1:
            gout = torch.tensor([0.75])
            gx = torch.full_like(x, float("nan"))
            lib.lp_grad(desc, x.data_ptr(), y.data_ptr(), runs[0][2].data_ptr(), gout.data_ptr(), gx.data_ptr())
    if chunks:
        assert n_chunks > 1 or chunks == 1
    for a, b in zip(*runs):
        assert torch.equal(a, b)                                         # bit-identical repeats
    ws, v, dv, loss = runs[0]
    num, den = _want_sums(x.numpy(), y.numpy(), len(dims), h1, p, tabs, periodic)
    part = ws.double().reshape(lines, n_chunks, 2).sum(dim=1).numpy()
    assert rel_l2(part[:, 0], num) <= 2e-6 and rel_l2(part[:, 1], den) <= 2e-6
    r = root and p != 1
    if relative:
        want_v = num ** (1 / p) / (den ** (1 / p) + eps) if r else num / (den + eps)
        want_dv = want_v / (p * num) if r else 1 / (den + eps)
    else:
        want_v = (konst * num) ** (1 / p) if r else konst * num
        want_dv = want_v / (p * num) if r else np.full(lines, konst)
    f = 1 / lines if mean else 1.0
    assert rel_l2(v.numpy(), want_v) <= 5e-6 and rel_l2(dv.numpy(), want_dv * f) <= 5e-6
    assert abs(float(loss) - f * want_v.sum()) <= 5e-6 * abs(f * want_v.sum())
    if not h1:
        e = x.numpy().astype(np.float64) - y.numpy()
        want_g = (want_dv * f * 0.75 * p).reshape((-1,) + (1,) * len(dims)) * np.abs(e) ** (p - 1) * np.sign(e)
        assert rel_l2(gx.numpy(), want_g) <= 5e-6


def test_refused_arguments_return_their_error():
    rng = np.random.default_rng(1)
    dims, periodic = (4, 6), (False, True)
    tabs = [torch.from_numpy(t) for t in _random_tables(rng, dims, periodic, (2, 2))]
    u = torch.zeros(2, 2, 4, 6)
    with engine_on_emulation() as lib:
        fdr.refused_stencil_arguments(lib)
        with pytest.raises(ValueError, match="tables for"):
            engine._band_apply(torch.zeros(1, 1, 4, 5), None, engine.BandTables(tabs, periodic, [(0, 1)] * 2), (), 1, False)
    with pytest.raises(AssertionError, match="outside its 7 bands"):
        engine.band_table(np.ones((9, 9)), False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine._band_apply(u, None, engine.BandTables(tabs, periodic, [(0, 1)] * 2), (), 1, False)


@pytest.mark.parametrize("name", fdr.EMU_BAND_KERNEL_CASES)
def test_band_kernel_edge_cases_of_the_gpu_tier(name):
    """the cases of tests/test_gpu_stencil_kernels.py the emulation finishes quickly, at the same two bars"""
    cfg = fdr.BAND_KERNEL_CASES[name]
    inputs = fdr.band_case_inputs(cfg, 91)
    with engine_on_emulation() as lib:
        got = fdr.run_band_case(lib, cfg, inputs)
    fdr.check_band_case(name, cfg, inputs, got)


@pytest.mark.parametrize("name", fdr.EMU_SUMS_KERNEL_CASES)
def test_loss_kernel_edge_cases_of_the_gpu_tier(name):
    cfg = fdr.SUMS_KERNEL_CASES[name]
    inputs = fdr.sums_case_inputs(cfg, 93)
    with engine_on_emulation() as lib:
        got = fdr.run_sums_case(lib, cfg, inputs)
        fdr.check_sums_case(name, cfg, inputs, got, lib)
        assert got["n_chunks"] == fdr.sob_plan(cfg["dims"], cfg["h1"], cfg["lines"], cfg["chunks"])[1]


@pytest.mark.parametrize("grid", [(1, 5, 6), (5, 2, 6), (5, 6, 3), (1, 1, 1)], ids=lambda g: "x".join(map(str, g)))
def test_finite_diff_tables_of_the_smallest_periodic_extents(grid):
    """the host's table builder owns the aliasing rule: D1 and D2 of every axis against the dense float64 matrices"""
    h = (0.5, 1.25, 0.75)
    u = torch.randn(2, 1, *grid, generator=torch.Generator().manual_seed(5))
    with engine_on_emulation():
        tabs = engine.finite_diff_tables(u.device, grid, h, (True,) * 3)
        for axis in range(3):
            for row in (0, 1):
                got = engine._band_apply(u, None, tabs, ((0, 0, 1.0, axis, row),), 1, False)
                want = fdr.apply_matrix(fdr.dense_matrix(grid[axis], h[axis], row + 1, True), u.double(), axis - 3)
                scale = float(want.abs().max())
                assert float((got.double() - want).abs().max()) <= 1e-5 * scale if scale else not got.any()
