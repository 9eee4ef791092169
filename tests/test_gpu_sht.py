"""GPU tier of the spherical-harmonic transforms (sc_kernels_sht.h behind neuraloperator_amd.RealSHT / InverseRealSHT):
forward and backward on the device against the float64 host restatement (tests/sht_reference.py) at bench.py's sfno
shape, a many-lines shape and an odd one; SphericalConv against the fixtures recorded from the verbatim reference layer
(tests/golden/sphconv_*.npz); bit-identical repeat launches."""
import os

import numpy as np
import pytest
import torch

import sht_reference as sr
from engine_runner import rel_l2

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda:0")

# lead, nlat, nlon, lmax, mmax, grid, norm
SHAPES = [((8, 32), 128, 256, 64, 64, "equiangular", "ortho"),           # bench.py sfno_extra
          ((4096,), 32, 64, 16, 16, "legendre-gauss", "ortho"),          # many lines
          ((3, 5), 33, 70, 40, 21, "legendre-gauss", "schmidt")]         # odd, lmax > nlat, partial tiles


@pytest.mark.parametrize("shape", SHAPES, ids=["bench", "lines4096", "odd"])
def test_transforms_forward_backward_on_device(shape):
    from neuraloperator_amd import InverseRealSHT, RealSHT
    lead, nlat, nlon, lmax, mmax, grid, norm = shape
    g = torch.Generator().manual_seed(11)
    x = torch.randn(*lead, nlat, nlon, generator=g)
    gc = torch.complex(torch.randn(*lead, lmax, mmax, generator=g), torch.randn(*lead, lmax, mmax, generator=g))
    gy = torch.randn(*lead, nlat, nlon, generator=g)
    fwd = RealSHT(nlat, nlon, lmax, mmax, grid=grid, norm=norm).to(DEV)
    inv = InverseRealSHT(nlat, nlon, lmax, mmax, grid=grid, norm=norm).to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    c = fwd(xd)
    c.backward(gc.to(DEV))
    cd = c.detach().requires_grad_(True)
    y = inv(cd)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    xr = x.double().requires_grad_(True)
    cr = sr.f64_sht(xr, lmax, mmax, grid, norm)
    cr.backward(gc.to(torch.complex128))
    c64 = c.detach().cpu().to(torch.complex128).requires_grad_(True)
    yr = sr.f64_isht(c64, nlat, nlon, grid, norm)
    yr.backward(gy.double())
    assert rel_l2(c.detach().cpu().numpy(), cr.detach().numpy()) <= 2e-6
    assert rel_l2(y.detach().cpu().numpy(), yr.detach().numpy()) <= 2e-6
    assert rel_l2(xd.grad.cpu().numpy(), xr.grad.numpy()) <= 1e-5
    assert rel_l2(cd.grad.cpu().numpy(), c64.grad.numpy()) <= 1e-5


@pytest.mark.parametrize("name", sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("sphconv_")))
def test_spherical_conv_against_reference_fixtures(name):
    from neuraloperator_amd import SphericalConv
    rec = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    fac = "cp" if "_cp_" in name else "dense"
    grid = "legendre-gauss" if "_lg" in name else "equiangular"
    x, g = torch.from_numpy(rec["x"]), torch.from_numpy(rec["g"])
    state = {k[2:]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("p:")}
    ci, co = int(x.shape[1]), int(g.shape[1])
    conv = SphericalConv(ci, co, tuple(int(v) for v in rec["n_modes"]), factorization=fac, rank=0.5, sht_grids=grid)
    conv.load_state_dict(state, strict=True)
    conv = conv.to(DEV)
    xd = x.to(DEV).requires_grad_(True)
    out_shape = tuple(g.shape[-2:]) if tuple(g.shape[-2:]) != tuple(x.shape[-2:]) else None
    y = conv(xd, output_shape=out_shape) if out_shape else conv(xd)
    y.backward(g.to(DEV))
    torch.cuda.synchronize()
    errs = {"y": rel_l2(y.detach().cpu().numpy(), rec["y"]), "gx": rel_l2(xd.grad.cpu().numpy(), rec["gx"])}
    for n, p in conv.named_parameters():
        errs[n] = rel_l2(p.grad.cpu().numpy(), rec["g:" + n])
    assert all(v <= 1e-5 for v in errs.values()), errs


def test_two_launches_are_bit_identical():
    from neuraloperator_amd import InverseRealSHT, RealSHT
    g = torch.Generator().manual_seed(3)
    x = torch.randn(8, 32, 128, 256, generator=g).to(DEV)
    fwd, inv = RealSHT(128, 256, 64, 64).to(DEV), InverseRealSHT(128, 256, 64, 64).to(DEV)
    runs = []
    for _ in range(2):
        xi = x.clone().requires_grad_(True)
        c = fwd(xi)
        y = inv(c)
        y.square().sum().backward()
        torch.cuda.synchronize()
        runs.append((c.detach().cpu(), y.detach().cpu(), xi.grad.cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_a_table_left_on_the_host_is_refused():
    """RealSHT(...) used on a device tensor without .to(device): the host table must raise, never reach a kernel."""
    from neuraloperator_amd import InverseRealSHT, RealSHT
    x = torch.randn(2, 16, 32, device=DEV)
    with pytest.raises(RuntimeError, match="Legendre table"):
        RealSHT(16, 32, 8, 8)(x)
    with pytest.raises(RuntimeError, match="Legendre table"):
        InverseRealSHT(16, 32, 8, 8)(torch.zeros(2, 8, 8, dtype=torch.complex64, device=DEV))
