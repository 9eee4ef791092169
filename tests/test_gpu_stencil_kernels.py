"""GPU tier: the banded stencil and loss kernels (sc_kernels_stencil.h: k_band_apply, k_sobolev_partial, k_loss_finish,
k_lp_grad) at their tile, chunk and pass edges on an MI355X, driven through the C-ABI with free-standing descriptors
(finite_diff_reference.run_band / run_sums_case) against a float64 numpy evaluation of the kernels' own formulas.

BAND_KERNEL_CASES (k_band_apply, tile 32 rows x 64 columns, halo 3):
  a  extents one short of, at and one past the tile on both axes, (1, 65) and (33, 1); periodic, then clamped
  b  the smallest extents in turn on each internal axis: periodic 1, 2, 3 (the taps alias), clamped 4; random tables
     here, the FiniteDiff module against dense float64 matrices below (the host's table builder owns the aliasing rule)
  c  axis-0 taps read from global memory: (7, 33, 65), axis 0 clamped / periodic, an all-zero table row, u2 fused
  d  twelve slots over 3 sources x 3 outputs, a term-less output, scale with scale_mul, out-major strides, gaps behind
     every output
  e  4099 groups of (3, 5)
SUMS_KERNEL_CASES (k_sobolev_partial / k_loss_finish / k_lp_grad):
  a  chunk plans of one line: 300 units cut into 1, 5, 256, 257 -> 150, 300 and the default number of chunks (the
     strided chunk loop of the finish kernel, a ragged last chunk), 16-byte and scalar route; H1 over 300 tiles
  b  passes of the finish kernel: 257 and 300 lines of one chunk, 300 lines of 3 chunks (sub 4), 65 of 5 (sub 8)
  c  1, 2, 3, 4, 1023, 1024, 1025, 4100 points per line; x, y, gx in turn one float into aligned storage
  d  p 1, 2, 3, 6 x relative / absolute x root / none x mean / sum for Lp; the same for H1 at (33, 65), at
     (4, 33, 65) with axis 0 clamped and at (3, 33, 65) with axis 0 periodic (a clamped axis of 3 points is refused)
  e  a line with x = y exactly and a line with y = 0 among ordinary ones
Every compared tensor meets the project's rel-L2 (1e-5) and, per element, |got - want| <= gamma_N A with A and N from
finite_diff_reference (derived from the kernel source, not measured); where A is 0 the value is exactly 0.  The loss
scalars are sums of non-negative terms (H1: of squares of stencils, A from the stencils' absolute values): their
bound is relative and adds the chunk sum, the finish arithmetic and the sum of the lines.  The root with p other than
2 is powf, whose error no document of the ROCm installation states: v, dv and the loss of those cases are held to 1e-5
only."""
import numpy as np
import pytest
import torch

import finite_diff_reference as fdr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _lib():
    from neuraloperator_amd import _lib
    return _lib.get_lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("name", sorted(fdr.BAND_KERNEL_CASES))
def test_band_apply_edges_against_float64(name):
    cfg = fdr.BAND_KERNEL_CASES[name]
    inputs = fdr.band_case_inputs(cfg, 91)
    got = fdr.run_band_case(_lib(), cfg, inputs, DEV, _stream())
    fdr.check_band_case(name, cfg, inputs, got)


@pytest.mark.parametrize("name", ["a_33x65_periodic", "a_33x65_clamped", "c_7x33x65_axis0_periodic_zero_row",
                                  "d_twelve_slots", "e_4099_groups_3x5"])
def test_band_apply_twice_gives_the_same_bits(name):
    cfg = fdr.BAND_KERNEL_CASES[name]
    inputs = fdr.band_case_inputs(cfg, 92)
    a, b = (fdr.run_band_case(_lib(), cfg, inputs, DEV, _stream()) for _ in range(2))
    assert torch.equal(a, b)


SMALL_GRIDS = [((1, 5, 6), (True,) * 3), ((2, 5, 6), (True,) * 3), ((3, 5, 6), (True,) * 3), ((5, 1, 6), (True,) * 3),
               ((5, 2, 6), (True,) * 3), ((5, 3, 6), (True,) * 3), ((5, 6, 1), (True,) * 3), ((5, 6, 2), (True,) * 3),
               ((5, 6, 3), (True,) * 3), ((1, 1, 1), (True,) * 3), ((4, 5, 6), (False, True, True)),
               ((5, 4, 6), (True, False, True)), ((5, 6, 4), (True, True, False)), ((4, 4, 4), (False,) * 3)]


@pytest.mark.parametrize("grid,periodic", SMALL_GRIDS, ids=["x".join(map(str, g)) + ("" if all(p) else "-clamped")
                                                            for g, p in SMALL_GRIDS])
def test_finite_diff_module_on_the_smallest_extents_against_dense_matrices(grid, periodic):
    from neuraloperator_amd import FiniteDiff
    h = (0.5, 1.25, 0.75)
    fd = FiniteDiff(3, h=h, **{"periodic_in_" + "xyz"[a]: periodic[a] for a in range(3)})
    want = fdr.F64FiniteDiff(3, h, periodic)
    u = torch.randn(2, 3, *grid, generator=torch.Generator().manual_seed(5))
    ud = u.to(DEV)
    errs = {}
    for m, kw in (("dx", {}), ("dy", {}), ("dz", {}), ("dx", dict(order=2)), ("dy", dict(order=2)),
                  ("dz", dict(order=2)), ("laplacian", {})):
        a, b = getattr(fd, m)(ud, **kw).cpu(), getattr(want, m)(u, **kw)
        key = m + str(kw.get("order", ""))
        errs[key] = fdr.rel_l2(a, b) if float(b.abs().max()) > 0 else float(a.abs().max())
    print(grid, periodic, {k: f"{e:.1e}" for k, e in errs.items()})
    assert all(e <= 1e-5 for e in errs.values()), errs


def test_the_chunk_plans_the_cases_are_cut_for():
    """the chunk count read back from sc_sobolev_workspace_bytes against what sob_plan must cut: which case reaches
    sub = 256 with the strided chunk loop, which a ragged last chunk, which several passes of the finish kernel"""
    lib = _lib()
    seen = {}
    for name, cfg in fdr.SUMS_KERNEL_CASES.items():
        desc = lib.sobolev_desc(dims=cfg["dims"], periodic=cfg["periodic"], lines=cfg["lines"], h1=cfg["h1"], p=cfg["p"],
                                chunks=cfg["chunks"])
        n = lib.sobolev_workspace_bytes(desc) // (8 * cfg["lines"])
        if cfg["chunks"]:
            assert n == fdr.sob_plan(cfg["dims"], cfg["h1"], cfg["lines"], cfg["chunks"])[1], name
        seen[name] = (n,) + fdr.finish_plan(cfg["lines"], n)
    refused = lib.sobolev_desc(dims=(3, 33, 65), periodic=(False, True, True), lines=3, h1=True, chunks=2)
    assert lib.sobolev_workspace_bytes(refused) == 0                       # extent 3 cannot be clamped: see group d
    for tag in ("vec", "scalar"):
        assert seen[f"a_lp_{tag}_chunks1"][:2] == (1, 1)
        assert seen[f"a_lp_{tag}_chunks5"][:2] == (5, 8)                   # 60 (61) units each, the last chunk ragged
        assert seen[f"a_lp_{tag}_chunks0"][0] >= 1
    assert seen["a_lp_vec_chunks256"] == (150, 256, 1, 1)                  # 300 units, 2 each: 256 asked for, 150 cut
    assert seen["a_lp_vec_chunks257"] == (150, 256, 1, 1)
    assert seen["a_lp_vec_chunks300"] == (300, 256, 1, 2)                  # sub = 256, threads 0 .. 43 sum two chunks
    for ch in (256, 257, 300):                                             # 301 units, the last one of 7 points: 150
        assert seen[f"a_lp_scalar_chunks{ch}"] == (151, 256, 1, 1)         # chunks of 2 and one of 1
    assert seen["a_h1_640x960_chunks7"][:2] == (7, 8)                      # 43 tiles each, the last chunk 42
    assert seen["a_h1_640x960_chunks299"][:2] == (150, 256)
    assert seen["a_h1_640x960_chunks300"] == (300, 256, 1, 2)
    assert seen["b_lines257_chunks1"] == (1, 1, 2, 1) and seen["b_lines300_chunks1"] == (1, 1, 2, 1)
    assert seen["b_lines300_chunks3"] == (3, 4, 5, 1) and seen["b_h1_lines300_chunks3"] == (3, 4, 5, 1)
    assert seen["b_lines65_chunks5"] == (5, 8, 3, 1)


@pytest.mark.parametrize("name", sorted(fdr.SUMS_KERNEL_CASES))
def test_loss_kernels_against_float64(name):
    cfg = fdr.SUMS_KERNEL_CASES[name]
    inputs = fdr.sums_case_inputs(cfg, 93)
    lib = _lib()
    got = fdr.run_sums_case(lib, cfg, inputs, DEV, _stream())
    fdr.check_sums_case(name, cfg, inputs, got, lib, DEV, _stream())


@pytest.mark.parametrize("name", ["a_lp_vec_chunks300", "a_lp_scalar_chunks257", "a_h1_640x960_chunks300",
                                  "b_lines300_chunks3", "b_lines65_chunks5"])
def test_loss_kernels_twice_give_the_same_bits(name):
    cfg = fdr.SUMS_KERNEL_CASES[name]
    inputs = fdr.sums_case_inputs(cfg, 94)
    a, b = (fdr.run_sums_case(_lib(), cfg, inputs, DEV, _stream()) for _ in range(2))
    for k in ("ws", "v", "dv", "loss") + (() if cfg["h1"] else ("gx",)):
        assert torch.equal(a[k], b[k]), k


def test_refused_arguments_return_their_error_on_the_device_library():
    fdr.refused_stencil_arguments(_lib(), DEV)
