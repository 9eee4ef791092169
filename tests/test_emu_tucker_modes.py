"""CPU tier: T[f, g, x, y] = sum_{c, d} core[f, g, c, d] U_x[x, c] U_y[y, d] in one launch each way
(sc_kernels_tucker.h; the batch-independent part of _contract_tucker, spectral_convolution.py:76-103) in host emulation
against torch's complex128 einsum and its autograd; the sizes of BASELINE configs[2] (ranks (36, 36, 36, 19), kept
64 x 33) at a reduced number of (f, g) pairs, ragged small sizes, the size limits.  Then the rows of
factor_reference.TUCKER_CASES the emulator can afford (at least one per path code of sc_tucker_modes_path): route
asserted, guarded buffers, rel-L2 and the element bound gamma_N S against the float64 reference written out by hand."""
import numpy as np
import pytest
import torch

import factor_reference as fr
from engine_runner import emu_lib, rel_l2


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


def _c(*shape, g):
    return torch.complex(torch.randn(*shape, generator=g), torch.randn(*shape, generator=g))


@pytest.mark.parametrize("fg,rx,ry,mx,my", [(40, 36, 19, 64, 33), (7, 3, 5, 6, 4), (600, 4, 2, 8, 5), (3, 64, 16, 64, 64)])
def test_tucker_mode_factors(lib, fg, rx, ry, mx, my):
    g = torch.Generator().manual_seed(fg)
    core, ux, uy, gt = _c(fg, rx, ry, g=g), _c(mx, rx, g=g), _c(my, ry, g=g), _c(fg, mx, my, g=g)
    assert lib.tucker_modes_supported(fg, rx, ry, mx, my)
    t = torch.full((fg, mx, my), float("nan"), dtype=torch.complex64)
    p = lambda z: torch.view_as_real(z).data_ptr()
    lib.tucker_modes_forward(fg, rx, ry, mx, my, p(core), p(ux), p(uy), p(t), 0)
    cd, ad, bd = (z.to(torch.complex128).requires_grad_(True) for z in (core, ux, uy))
    ref = torch.einsum("ncd,xc,yd->nxy", cd, ad, bd)
    assert rel_l2(t.numpy(), ref.detach().numpy()) < 2e-6
    ref.backward(gt.to(torch.complex128))
    gc, ga, gb = torch.empty_like(core), torch.empty_like(ux), torch.empty_like(uy)
    ws = torch.empty(lib.tucker_modes_workspace_bytes(fg, rx, ry, mx, my), dtype=torch.uint8)
    lib.tucker_modes_backward(fg, rx, ry, mx, my, p(core), p(ux), p(uy), p(gt), p(gc), p(ga), p(gb), ws.data_ptr(), 0)
    assert rel_l2(gc.numpy(), cd.grad.numpy()) < 5e-6
    assert rel_l2(ga.numpy(), ad.grad.numpy()) < 5e-6
    assert rel_l2(gb.numpy(), bd.grad.numpy()) < 5e-6


def test_limits(lib):
    assert lib.tucker_modes_supported(10, 64, 16, 64, 64)
    assert not lib.tucker_modes_supported(10, 36, 19, 128, 33)      # more than 64 modes along a dim
    assert not lib.tucker_modes_supported(10, 36, 40, 64, 33)       # My Ry beyond a thread set
    assert lib.tucker_modes_workspace_bytes(10, 36, 19, 128, 33) == 0


@pytest.mark.parametrize("name", fr.emu_rows(fr.TUCKER_CASES))
def test_tucker_table_on_guarded_buffers(lib, name):
    _, stats = fr.run_tucker(lib, name, torch.device("cpu"))
    assert set(stats) == {"t", "gcore", "gux", "guy"}


@pytest.mark.parametrize("name", sorted(fr.TUCKER_REFUSED))
def test_refused_shapes_fail_loudly_and_write_nothing(lib, name):
    fr.run_tucker_refused(lib, name, torch.device("cpu"))


def test_every_route_has_a_row_and_the_emulator_one_per_instantiation():
    full, emu = fr.coverage(), fr.coverage(emu_only=True)
    assert {p for k, p in full if k == "tucker"} == set(fr.TUCKER_PATHS) == {p for k, p in emu if k == "tucker"}
    assert all(rows for rows in emu.values())


def test_the_route_mirror_at_the_layout_edge():
    """the padded backward layout of the rows the issue names, in bytes, and the side of 150 KB they fall on"""
    assert fr.tucker_layout_bytes(64, 20, 16, 51) == 92864 and fr.tucker_layout_bytes(64, 16, 64, 56) == 147328
    assert fr.tucker_layout_bytes(64, 16, 64, 64) > fr.LDS_EDGE >= fr.tucker_vector_bytes(64, 16, 64, 64)
    for c in fr.TUCKER_CASES.values():
        assert fr.tucker_path(c["fg"], c["rx"], c["ry"], c["mx"], c["my"]) == c["path"]


def test_the_written_out_gradients_are_those_of_autograd():
    """the float64 reference uses no autograd, so that every gradient can be bounded; here it meets torch's"""
    name = "ragged"
    core, ux, uy, gt = (z.to(torch.complex128) for z in fr.tucker_inputs(name))
    cd, ad, bd = (z.clone().requires_grad_(True) for z in (core, ux, uy))
    out = torch.einsum("ncd,xc,yd->nxy", cd, ad, bd)
    out.backward(gt)
    ref, S = fr.tucker_reference(name)
    for got, key in ((out.detach(), "t"), (cd.grad, "gcore"), (ad.grad, "gux"), (bd.grad, "guy")):
        assert rel_l2(got.numpy(), ref[key]) < 1e-14
        assert (np.abs(ref[key]) <= S[key] * (1 + 1e-12)).all()


@pytest.mark.parametrize("name", sorted(fr.TUCKER_CASES))
def test_the_reference_rounded_to_fp32_sits_inside_its_own_bound(name):
    """every row, the device-only ones too: gamma_N S is not below what fp32 can hold"""
    c = fr.TUCKER_CASES[name]
    ref, S = fr.tucker_reference(name)
    N = fr.tucker_counts(c, min(c["fg"], fr.TUCKER_WG_CAP))
    for key in ref:
        r32 = ref[key].astype(np.complex64).astype(np.complex128)
        assert (np.maximum(np.abs((r32 - ref[key]).real), np.abs((r32 - ref[key]).imag)) <= fr.gamma(N[key]) * S[key]).all()
