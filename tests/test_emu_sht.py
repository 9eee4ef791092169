"""The Legendre kernels of the spherical-harmonic transforms (sc_kernels_sht.h: sc_legendre_analysis / _synthesis) in host
emulation, against a float64 numpy einsum with the same tables: both grids, the three norms, Condon-Shortley phase on
and off, odd nlat, mmax below / above lmax, lmax above nlat, more than one 64-column m group and one 16-row block (lmax = mmax = 72:
the second group's synthesis starts at l = 64), line counts that are not a multiple of the per-lane tile; the adjoint
identity of each kernel; size errors; a table off the operand's device is refused before any launch.  The quick cases
of the GPU tier (tests/test_gpu_sht_kernels.py: sht_reference.EMU_SHT_KERNEL_CASES) run here at the same two bars."""
import numpy as np
import pytest
import torch

import sht_reference as sr
from emu_engine import engine_on_emulation
from engine_runner import rel_l2
from sht_reference import crandn as _crandn
from neuraloperator_amd import _lib, engine
from neuraloperator_amd.harmonics import _table

# grid, norm, csphase, nlat, lmax, mmax, lines
CASES = [("equiangular", "ortho", True, 9, 6, 4, 1),
         ("legendre-gauss", "four-pi", False, 8, 5, 7, 5),
         ("equiangular", "schmidt", True, 6, 9, 5, 3),
         ("legendre-gauss", "schmidt", False, 7, 7, 7, 6),
         ("equiangular", "four-pi", False, 5, 3, 70, 2),
         ("legendre-gauss", "ortho", True, 21, 18, 10, 9),
         ("equiangular", "ortho", False, 17, 20, 9, 4),
         ("equiangular", "ortho", True, 5, 72, 72, 2)]          # a second 64-column group with a non-empty sum


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0][:2]}-{c[1]}-cs{int(c[2])}-{c[3]}x{c[4]}x{c[5]}-L{c[6]}" for c in CASES])
def test_legendre_kernels_match_float64(case):
    grid, norm, cs, nlat, lmax, mmax, lines = case
    g = torch.Generator().manual_seed(nlat * 1000 + lmax * 10 + mmax)
    ta = _table(nlat, lmax, mmax, grid, norm, cs, analysis=True)
    ts = _table(nlat, lmax, mmax, grid, norm, cs, analysis=False)
    assert tuple(ta.shape) == (lmax, nlat, mmax) and ta.dtype == torch.float32
    for l in range(lmax):                                   # the zero triangle the kernels skip
        assert torch.all(ta[l, :, l + 1:] == 0) and torch.all(ts[l, :, l + 1:] == 0)
    x = _crandn(g, lines, nlat, mmax)
    c = _crandn(g, lines, lmax, mmax)
    with engine_on_emulation():
        ca = engine.LegendreAnalysisFn.apply(x, ta)
        xs = engine.LegendreSynthesisFn.apply(c, ts)
    want_c = np.einsum("nkm,lkm->nlm", x.numpy().astype(np.complex128), ta.numpy().astype(np.float64))
    want_x = np.einsum("nlm,lkm->nkm", c.numpy().astype(np.complex128), ts.numpy().astype(np.float64))
    assert ca.shape == (lines, lmax, mmax) and xs.shape == (lines, nlat, mmax)
    assert rel_l2(ca.numpy(), want_c) < 2e-6
    assert rel_l2(xs.numpy(), want_x) < 2e-6
    for l in range(lmax):
        assert torch.all(ca[:, l, l + 1:] == 0)            # written in full, zeros below the diagonal


@pytest.mark.parametrize("case", CASES[1:4], ids=["lg-fourpi", "eq-schmidt", "lg-schmidt"])
def test_legendre_kernels_are_each_others_adjoint(case):
    """<A x, y> = <x, A^T y> with A = analysis (T), A^T = synthesis with the same table, and the other way round;
    the autograd of each Function is that identity."""
    grid, norm, cs, nlat, lmax, mmax, lines = case
    g = torch.Generator().manual_seed(7)
    dot = lambda a, b: float(torch.sum(a.conj() * b).real)
    for analysis in (True, False):
        tab = _table(nlat, lmax, mmax, grid, norm, cs, analysis=analysis)
        x = _crandn(g, lines, nlat, mmax).requires_grad_(True)
        y = _crandn(g, lines, lmax, mmax)
        c = _crandn(g, lines, lmax, mmax).requires_grad_(True)
        z = _crandn(g, lines, nlat, mmax)
        with engine_on_emulation():
            ax = engine.LegendreAnalysisFn.apply(x, tab)
            aty = engine.LegendreSynthesisFn.apply(y, tab)
            sc = engine.LegendreSynthesisFn.apply(c, tab)
            stz = engine.LegendreAnalysisFn.apply(z, tab)
            (ax.conj() * y).real.sum().backward()
            (sc.conj() * z).real.sum().backward()
        lhs, rhs = dot(ax.detach(), y), dot(x.detach(), aty)
        assert abs(lhs - rhs) <= 1e-5 * (abs(lhs) + abs(rhs))
        lhs, rhs = dot(sc.detach(), z), dot(c.detach(), stz)
        assert abs(lhs - rhs) <= 1e-5 * (abs(lhs) + abs(rhs))
        assert rel_l2(x.grad.numpy(), aty.numpy()) < 1e-6           # d/dx of Re<Ax, y> = A^T y
        assert rel_l2(c.grad.numpy(), stz.numpy()) < 1e-6


def test_legendre_entry_points_reject_bad_sizes():
    with engine_on_emulation() as lib:
        x = torch.zeros(2, 4, 3, dtype=torch.complex64)
        tab = torch.zeros(4, 4, 3)
        sr.refused_legendre_arguments(lib)
        with pytest.raises(ValueError):
            engine.LegendreAnalysisFn.apply(x, tab[:, :3].contiguous())    # nlat of the table differs
        with pytest.raises(ValueError):
            engine.LegendreSynthesisFn.apply(x, tab.double())


def test_legendre_refuses_a_table_off_the_operands_device(monkeypatch):
    """Both pointers reach the kernel: a host table beside a device operand would be read by the GPU.  The table is
    checked like the operand (no emulation patch here: the stub stands in for the device test and records its calls)."""
    x = torch.zeros(2, 4, 3, dtype=torch.complex64)
    tab = torch.zeros(4, 4, 3)
    seen = []

    def require_gpu(t, what="input"):
        seen.append(what)
        if "table" in what:
            raise RuntimeError(f"{what} is on {t.device}")
    monkeypatch.setattr(engine, "_require_gpu", require_gpu)
    for fn in (engine.LegendreAnalysisFn, engine.LegendreSynthesisFn):
        seen.clear()
        with pytest.raises(RuntimeError, match="table"):
            fn.apply(x, tab)
        assert seen[-2:] == ["Legendre operand", "Legendre table"]
    monkeypatch.setattr(engine, "_require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(_lib, "_LIB", None)              # a launch would need the library: none must happen
    with pytest.raises(ValueError, match="device"):
        engine.LegendreAnalysisFn.apply(x, tab.to("meta"))
    with pytest.raises(ValueError, match="device"):
        engine.LegendreSynthesisFn.apply(x, tab.to("meta"))


@pytest.mark.parametrize("name", sr.EMU_SHT_KERNEL_CASES)
def test_kernel_edge_cases_of_the_gpu_tier(name):
    """the cases of tests/test_gpu_sht_kernels.py the emulation finishes quickly, at the same two bars"""
    inputs = sr.sht_case_inputs(name, 91)
    with engine_on_emulation() as lib:
        got = sr.run_sht_case(lib, inputs)
    sr.check_sht_case(name, inputs, got)
