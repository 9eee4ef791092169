"""The public transform objects neuraloperator_amd.RealSHT / InverseRealSHT (engine in host emulation) and the
torch_harmonics stand-in: closed-form spherical harmonics, a band-limited round trip, autograd through both transforms
against the float64 restatement (tests/sht_reference.py), module plumbing, install_torch_harmonics()."""
import math
import sys
import types

import numpy as np
import pytest
import torch

import sht_reference as sr
from emu_engine import engine_on_emulation
from engine_runner import rel_l2
from neuraloperator_amd import InverseRealSHT, RealSHT, SphericalConv, install_torch_harmonics


@pytest.mark.parametrize("grid,nlat,nlon", [("equiangular", 33, 64), ("legendre-gauss", 24, 48)])
def test_closed_form_harmonics_give_one_coefficient(grid, nlat, nlon):
    """x = Re Y_l^m -> c[l, m] = 1/2 (m > 0) or 1 (m = 0), x = Im Y_l^m -> -i/2, all else 0; synthesis returns x."""
    from scipy.special import sph_harm_y
    from neuraloperator_amd.spherical import quadrature
    theta, _ = quadrature(nlat, grid)
    TH, PH = np.meshgrid(theta, 2 * math.pi * np.arange(nlon) / nlon, indexing="ij")
    lmax = mmax = 10
    fields, want = [], []
    for l, m in [(0, 0), (2, 0), (2, 1), (4, 3), (6, 6), (9, 2), (9, 9)]:
        Y = sph_harm_y(l, m, TH, PH)
        for part, f in (("re", Y.real), ("im", Y.imag)) if m else (("re", Y.real),):
            c = np.zeros((lmax, mmax), dtype=np.complex128)
            c[l, m] = 1.0 if m == 0 else (0.5 if part == "re" else -0.5j)
            fields.append(f)
            want.append(c)
    x = torch.from_numpy(np.stack(fields)).float()
    cw = np.stack(want)
    with engine_on_emulation():
        got = RealSHT(nlat, nlon, lmax, mmax, grid=grid)(x)
        back = InverseRealSHT(nlat, nlon, lmax, mmax, grid=grid)(torch.from_numpy(cw).to(torch.complex64))
    assert got.dtype == torch.complex64 and tuple(got.shape) == (len(fields), lmax, mmax)
    assert np.abs(got.numpy() - cw).max() < 5e-6
    assert back.dtype == torch.float32 and np.abs(back.numpy() - x.numpy()).max() < 5e-6


@pytest.mark.parametrize("grid,norm,cs", [("equiangular", "schmidt", True), ("legendre-gauss", "four-pi", False)])
def test_band_limited_round_trip(grid, norm, cs):
    nlat, nlon, lmax, mmax = (17, 32, 8, 8) if grid == "equiangular" else (12, 24, 12, 10)
    g = torch.Generator().manual_seed(2)
    c = torch.complex(torch.randn(3, lmax, mmax, generator=g), torch.randn(3, lmax, mmax, generator=g))
    for m in range(mmax):
        c[..., :m, m] = 0
    c[..., 0] = c[..., 0].real.to(torch.complex64)
    with engine_on_emulation():
        x = InverseRealSHT(nlat, nlon, lmax, mmax, grid=grid, norm=norm, csphase=cs)(c)
        c2 = RealSHT(nlat, nlon, lmax, mmax, grid=grid, norm=norm, csphase=cs)(x)
    assert rel_l2(x.numpy(), sr.f64_isht(c, nlat, nlon, grid, norm, cs).numpy()) < 2e-6
    assert rel_l2(c2.numpy(), sr.f64_sht(x, lmax, mmax, grid, norm, cs).numpy()) < 2e-6
    assert rel_l2(c2.numpy(), c.numpy()) < 1e-5


@pytest.mark.parametrize("grid,shape", [("equiangular", (9, 16, 6, 9, 18)), ("legendre-gauss", (8, 12, 8, 7, 10))])
def test_autograd_through_analysis_and_synthesis(grid, shape):
    """y = ISHT(w * SHT(x)) on two grids (the second one finer / coarser), mmax > nlon // 2 + 1 of the output grid in
    the second case: y and dL/dx against float64 torch autograd of the restatement."""
    nlat, nlon, lmax, nlat2, nlon2 = shape
    mmax = nlon // 2 + 1
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, nlat, nlon, generator=g)
    w = torch.complex(torch.randn(lmax, mmax, generator=g), torch.randn(lmax, mmax, generator=g))
    gy = torch.randn(2, 3, nlat2, nlon2, generator=g)
    fwd, inv = RealSHT(nlat, nlon, lmax, mmax, grid=grid), InverseRealSHT(nlat2, nlon2, lmax, mmax, grid=grid)
    xi = x.clone().requires_grad_(True)
    with engine_on_emulation():
        y = inv(fwd(xi) * w)
        y.backward(gy)
    xd = x.double().requires_grad_(True)
    yd = sr.f64_isht(sr.f64_sht(xd, lmax, mmax, grid) * w.to(torch.complex128), nlat2, nlon2, grid)
    yd.backward(gy.double())
    assert rel_l2(y.detach().numpy(), yd.detach().numpy()) < 2e-6
    assert rel_l2(xi.grad.numpy(), xd.grad.numpy()) < 1e-5


def test_module_plumbing():
    f = RealSHT(16, 32, lmax=8, mmax=6, grid="legendre-gauss")
    i = InverseRealSHT(16, 32)
    assert (i.lmax, i.mmax) == (16, 17)                    # defaults: nlat, nlon // 2 + 1
    assert f.state_dict() == {} and i.state_dict() == {}  # non-persistent tables
    for mod in (f, i):
        w = mod.weights
        assert mod.to(device="cpu") is mod and mod.to(dtype=torch.float32) is mod
        mod.to(dtype=torch.float64)
        assert mod.weights.dtype == torch.float32 and torch.equal(mod.weights, w)
    with pytest.raises(ValueError):
        RealSHT(16, 32, mmax=18)                           # more columns than the real transform has
    with pytest.raises(ValueError):
        f(torch.randn(2, 16, 30))
    for cast in ("half", "bfloat16"):                           # a 16-bit cast of the module keeps the fp32 table
        mod = RealSHT(16, 32, lmax=8, mmax=6)
        w = mod.weights.clone()
        getattr(mod, cast)()
        assert mod.weights.dtype == torch.float32 and torch.equal(mod.weights, w)
    conv = SphericalConv(3, 3, (8, 16))
    keys = set(conv.state_dict())
    with engine_on_emulation():
        conv(torch.randn(1, 3, 17, 32))
    assert set(conv.state_dict()) == keys


def test_install_torch_harmonics_is_idempotent_and_never_shadows(monkeypatch):
    monkeypatch.delitem(sys.modules, "torch_harmonics", raising=False)
    monkeypatch.setattr(sys, "path", list(sys.path))
    try:
        import torch_harmonics  # noqa: F401
        real = True
    except ImportError:
        real = False
    if not real:
        assert install_torch_harmonics() is True
        from torch_harmonics import InverseRealSHT as I2, RealSHT as R2
        assert (R2, I2) == (RealSHT, InverseRealSHT)
        mod = sys.modules["torch_harmonics"]
        assert install_torch_harmonics() is False and sys.modules["torch_harmonics"] is mod
    other = types.ModuleType("torch_harmonics")
    other.RealSHT = object
    monkeypatch.setitem(sys.modules, "torch_harmonics", other)
    assert install_torch_harmonics() is False
    assert sys.modules["torch_harmonics"] is other and other.RealSHT is object


def test_engine_flags_reach_the_transforms():
    """SphericalConv(engine_flags=...) reaches the 1-d plans of both transforms (as before the transforms had their own
    module), and the generic plans give the same layer."""
    from neuraloperator_amd import _lib, engine
    torch.manual_seed(0)
    x = torch.randn(2, 3, 17, 32)
    out = {}
    for flags in (0, _lib.SC_PLAN_FORCE_GENERIC):
        torch.manual_seed(1)
        conv = SphericalConv(3, 3, (8, 16), engine_flags=flags)
        with engine_on_emulation():
            out[flags] = conv(x)
            plans = {k[1]: k[4] for k in engine._PLANS}          # spatial -> flags
        assert plans[(32,)] == flags, plans
    assert rel_l2(out[_lib.SC_PLAN_FORCE_GENERIC].detach().numpy(), out[0].detach().numpy()) < 2e-6
