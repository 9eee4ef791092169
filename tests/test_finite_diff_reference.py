"""``neuraloperator_amd.FiniteDiff`` / ``LpLoss`` / ``H1Loss`` in the CPU tier (engine in host emulation) against the
fixtures recorded from the verbatim reference classes (tests/golden/finite_diff_*.npz, sobolev_loss_*.npz,
tests/record_finite_diff.py): every method's output and gradient at the project's fp32 parity bar 1e-5 -- rel-L2 for
fields, relative error for the scalar loss.  fp32 round-off of a 7-tap stencil and of sums over a few hundred points
sits near 1e-7, so the bar tests the formula, not the rounding (the reasoning of tests/test_fourier_diff_reference.py).
Where the reference exists: the live verbatim classes and the float64 helper against the fixtures at 1e-12, and the
verbatim classes in fp32, as users run them, against the engine at 1e-5.  Error paths and the keyword warning; double
backward of ``FiniteDiff.laplacian`` through the emulation."""
import os

import numpy as np
import pytest
import torch

import finite_diff_reference as fdr
from emu_engine import engine_on_emulation
from neuraloperator_amd import FiniteDiff, H1Loss, LpLoss

needs_reference = pytest.mark.skipif(not fdr.reference_available(), reason="the verbatim reference is not on this machine")
ENGINE = {"LpLoss": LpLoss, "H1Loss": H1Loss}


def _rec(name):
    return dict(np.load(os.path.join(fdr.GOLDEN, name + ".npz")))


def _fd(cls, name, **kw):
    grid, h, periodic = fdr.CASES[name]
    dim = len(grid)
    return cls(dim, h=h if dim > 1 else h[0], **{"periodic_in_" + "xyz"[a]: periodic[a] for a in range(dim)}, **kw)


def _leaves(rec, dtype):
    return (torch.from_numpy(rec["u"]).to(dtype).requires_grad_(True),
            torch.from_numpy(rec["v"]).to(dtype).requires_grad_(True))


def _scalar_err(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def _loss_errs(got, want):
    return {k: (fdr.rel_l2(t, want[k]) if k.endswith(":grad") else _scalar_err(t, want[k])) for k, t in got.items()}


@pytest.mark.parametrize("name", sorted(fdr.CASES))
def test_finite_diff_matches_the_recorded_reference(name):
    rec = _rec(name)
    u, v = _leaves(rec, torch.float32)
    with engine_on_emulation():
        got = fdr.run_all(_fd(FiniteDiff, name), u, v, int(rec["gseed"]), len(fdr.CASES[name][0]))
    assert sorted("ref:" + k for k in got) == sorted(k for k in rec if k.startswith("ref:"))
    errs = {k: fdr.rel_l2(t, rec["ref:" + k]) for k, t in got.items()}
    print(name, {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(t.dtype == torch.float32 for t in got.values())
    assert all(tuple(t.shape) == rec["ref:" + k].shape for k, t in got.items())
    assert all(e <= 1e-5 for e in errs.values()), errs


@pytest.mark.parametrize("name", sorted(fdr.LOSS_CASES))
def test_losses_match_the_recorded_reference(name):
    rec = _rec(name)
    x = torch.from_numpy(rec["x"]).requires_grad_(True)
    y = torch.from_numpy(rec["y"])
    with engine_on_emulation():
        got = fdr.run_losses(ENGINE, x, y, name)
    want = {k[4:]: v for k, v in rec.items() if k.startswith("ref:")}
    assert sorted(got) == sorted(want)
    assert all(t.dtype == torch.float32 for t in got.values())
    assert all(t.dim() == 0 for k, t in got.items() if not k.endswith(":grad"))
    errs = _loss_errs(got, want)
    print(name, {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(e <= 1e-5 for e in errs.values()), {k: e for k, e in errs.items() if e > 1e-5}


@needs_reference
@pytest.mark.parametrize("name", sorted(fdr.CASES))
def test_live_reference_helper_and_fixtures_agree(name):
    grid, h, periodic = fdr.CASES[name]
    dim = len(grid)
    rec = _rec(name)
    diff, _ = fdr.load_reference_losses()
    u, v = _leaves(rec, torch.float64)
    live = fdr.run_all(_fd(diff.FiniteDiff, name), u, v, int(rec["gseed"]), dim)
    u, v = _leaves(rec, torch.float64)
    helper = fdr.run_all(fdr.F64FiniteDiff(dim, h, periodic), u, v, int(rec["gseed"]), dim)
    u, v = _leaves(rec, torch.float32)
    live32 = fdr.run_all(_fd(diff.FiniteDiff, name), u, v, int(rec["gseed"]), dim)
    u, v = _leaves(rec, torch.float32)
    with engine_on_emulation():
        got = fdr.run_all(_fd(FiniteDiff, name), u, v, int(rec["gseed"]), dim)
    for k, t in live.items():
        assert fdr.rel_l2(t, rec["ref:" + k]) <= 1e-12, k               # the fixtures are what the reference computes
        assert fdr.rel_l2(helper[k], t) <= 1e-12, k
        assert fdr.rel_l2(got[k], live32[k]) <= 1e-5, k                  # fp32 against fp32, as users run it


@needs_reference
@pytest.mark.parametrize("name", sorted(fdr.LOSS_CASES))
def test_live_reference_losses_helper_and_fixtures_agree(name):
    rec = _rec(name)
    _, losses = fdr.load_reference_losses()
    ref = {"LpLoss": losses.LpLoss, "H1Loss": losses.H1Loss}
    want = {k[4:]: v for k, v in rec.items() if k.startswith("ref:")}
    x64 = lambda: torch.from_numpy(rec["x"]).double().requires_grad_(True)
    y = torch.from_numpy(rec["y"])
    live = fdr.run_losses(ref, x64(), y.double(), name)
    helper = fdr.f64_losses(x64(), y.double(), name)
    live32 = fdr.run_losses(ref, torch.from_numpy(rec["x"]).requires_grad_(True), y, name)
    with engine_on_emulation():
        got = fdr.run_losses(ENGINE, torch.from_numpy(rec["x"]).requires_grad_(True), y, name)
    assert max(_loss_errs(live, want).values()) <= 1e-12
    assert max(_loss_errs(helper, want).values()) <= 1e-12
    errs = _loss_errs(got, live32)
    assert max(errs.values()) <= 1e-5, {k: e for k, e in errs.items() if e > 1e-5}


def test_double_backward_of_the_laplacian_and_input_dtypes():
    """d/dc of |grad_u <lap u, c>|^2: the backward pass is the operator's transpose on the same kernel, so autograd
    differentiates it again; float64 / bfloat16 input is computed and returned in fp32"""
    g = torch.Generator().manual_seed(4)
    u = torch.randn(2, 7, 6, generator=g).requires_grad_(True)
    c = torch.randn(2, 7, 6, generator=g).requires_grad_(True)
    with engine_on_emulation():
        fd = FiniteDiff(2, h=(1.3, 0.7), periodic_in_x=False)
        gu, = torch.autograd.grad((fd.laplacian(u) * c).sum(), u, create_graph=True)
        gc, = torch.autograd.grad(gu.square().sum(), c)
        out64 = fd.dx(u.detach().double())
        out16 = fd.dx(u.detach().bfloat16())
        base = fd.dx(u.detach())
        wide = fd.dx(u.detach().bfloat16().float())
    h = fdr.F64FiniteDiff(2, (1.3, 0.7), (False, True))
    u64, c64 = u.detach().double().requires_grad_(True), c.detach().double().requires_grad_(True)
    gu64, = torch.autograd.grad((h.laplacian(u64) * c64).sum(), u64, create_graph=True)
    gc64, = torch.autograd.grad(gu64.square().sum(), c64)
    assert fdr.rel_l2(gu.detach(), gu64.detach()) <= 1e-5 and fdr.rel_l2(gc, gc64) <= 1e-5
    assert out64.dtype == out16.dtype == torch.float32
    assert torch.equal(out64, base) and torch.equal(out16, wide)


def test_finite_diff_error_paths_raise_what_the_reference_raises():
    with pytest.raises(ValueError, match="dim must be 1, 2, or 3"):
        FiniteDiff(4)
    with pytest.raises(ValueError, match="For 2D, h must be a float or a tuple of length 2"):
        FiniteDiff(2, h=(1.0, 2.0, 3.0))
    f1, f2, f3 = FiniteDiff(1, h=0.5), FiniteDiff(2), FiniteDiff(3, h=[1, 2, 3], periodic_in_y=False)
    assert f1.h == (0.5,) and f2.h == (1.0, 1.0) and f3.h == (1, 2, 3)
    assert not hasattr(f1, "periodic_in_y") and not hasattr(f2, "periodic_in_z") and f3.periodic_in_y is False
    u1, u2 = torch.zeros(2, 8), torch.zeros(2, 2, 8, 8)
    with pytest.raises(ValueError, match="dy is only available for 2D and 3D"):
        f1.dy(u1)
    with pytest.raises(ValueError, match="dz is only available for 3D"):
        f2.dz(u2)
    with pytest.raises(ValueError, match="Curl is not defined for 1D"):
        f1.curl(u1)
    with pytest.raises(ValueError, match="Input must be a 2D vector field with 2 components"):
        f2.curl(torch.zeros(3, 8, 8))
    with pytest.raises(ValueError, match="Input must be a 2D vector field with 2 components"):
        f2.divergence(torch.zeros(3, 8, 8))
    with pytest.raises(ValueError, match="Input must be a 3D vector field with 3 components"):
        f3.curl(torch.zeros(2, 4, 4, 4))
    with pytest.raises(ValueError, match="Only 1st and 2nd order derivatives currently supported"):
        f2.dx(u2, order=3)
    with pytest.raises(ValueError, match="non-periodic axis needs at least 4 points"):
        FiniteDiff(1, periodic_in_x=False).dx(torch.zeros(2, 3))           # the reference: IndexError
    with pytest.raises(RuntimeError, match="no CPU path"):
        f2.dx(u2)                                                          # the product has no host fall-back


def test_loss_constructors_error_paths_and_the_keyword_warning():
    lp, h1 = LpLoss(d=2, p=3, measure=2.0, reduction="mean"), H1Loss(d=3, measure=[1.0, 2.0, 3.0], periodic_in_y=False)
    assert lp.name == "L3_2Dloss" and h1.name == "H1_3DLoss"
    assert lp.measure == [2.0, 2.0] and h1.measure == [1.0, 2.0, 3.0] and lp.eps == h1.eps == 1e-8
    assert (h1.periodic_in_x, h1.periodic_in_y, h1.periodic_in_z) == (True, False, True)
    assert lp.uniform_quadrature(torch.zeros(1, 4, 8)) == [0.5, 0.25]
    assert h1.uniform_quadrature(torch.zeros(2, 4, 8)) == [0.5, 0.5, 0.375]
    with pytest.raises(AssertionError, match="expected `reduction`"):
        LpLoss(reduction="max")
    with pytest.raises(AssertionError, match="only implemented for 1, 2, and 3-D"):
        H1Loss(d=4)
    with pytest.raises(ValueError, match="integer >= 1"):
        LpLoss(p=0)
    x, y = torch.zeros(2, 6, 6), torch.ones(2, 6, 6)
    with pytest.raises(RuntimeError, match="no CPU path"):
        LpLoss(d=2)(x, y)
    with pytest.raises(RuntimeError, match="no CPU path"):
        H1Loss(d=2)(x, y)
    with pytest.raises(ValueError, match="differ in shape"):
        LpLoss(d=2)(x, y[:1])
    with pytest.raises(NotImplementedError, match="prediction only"):
        H1Loss(d=2)(x, y.clone().requires_grad_(True))
    with engine_on_emulation():
        with pytest.raises(ValueError, match="non-periodic axis needs at least 4 points"):
            H1Loss(d=2, periodic_in_y=False)(torch.zeros(2, 6, 3), torch.ones(2, 6, 3))
        with pytest.warns(UserWarning, match=r"H1Loss.__call__\(\) received unexpected keyword arguments: \['extra'\]"):
            a = H1Loss(d=2)(x, y, extra=1)
        with pytest.warns(UserWarning, match=r"LpLoss.__call__\(\) received unexpected keyword arguments: \['x'\]"):
            b = LpLoss(d=2)(x, y, x=None)
        xg = x.clone().requires_grad_(True)
        loss = H1Loss(d=2)(xg, y)
        w = torch.ones((), requires_grad=True)
        g1, = torch.autograd.grad(loss, xg, grad_outputs=w, create_graph=True)
        with pytest.raises(RuntimeError, match="once_differentiable"):
            g1.sum().backward()
    assert a.dim() == b.dim() == 0 and a.dtype == torch.float32
    assert abs(float(a) - 2.0) < 1e-5 and abs(float(b) - 2.0) < 1e-5        # ||0 - 1|| / ||1|| per line, two lines
