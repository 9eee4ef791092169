"""``neuraloperator_amd.FourierDiff`` in the CPU tier (engine in host emulation) against the fixtures recorded from
the verbatim reference class (tests/golden/fourier_diff_*.npz, tests/record_fourier_diff.py): every method's output and
``u.grad`` / ``v.grad`` at the project's fp32 parity bar 1e-5 (fp32 round-off sits near 2e-7 at these grids, so the bar
tests the formula, not the rounding).  Where the reference exists: the same cases live against the verbatim class,
and the float64 helper restatement against it at 1e-12.  The error paths raise what the reference raises."""
import os

import numpy as np
import pytest
import torch

import fourier_diff_reference as fr
from emu_engine import engine_on_emulation
from neuraloperator_amd import FourierDiff

needs_reference = pytest.mark.skipif(not fr.reference_available(), reason="the verbatim reference is not on this machine")


def _leaves(rec, dtype):
    return (torch.from_numpy(rec["u"]).to(dtype).requires_grad_(True),
            torch.from_numpy(rec["v"]).to(dtype).requires_grad_(True))


def _engine_results(name):
    grid, L, ratio = fr.CASES[name]
    rec = dict(np.load(os.path.join(fr.GOLDEN, name + ".npz")))
    u, v = _leaves(rec, torch.float32)
    with engine_on_emulation():
        fd = FourierDiff(len(grid), L=L if len(grid) > 1 else L[0], low_pass_filter_ratio=ratio)
        got = fr.run_all(fd, u, v, int(rec["gseed"]), len(grid))
    return rec, got


@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_engine_matches_the_recorded_reference(name):
    rec, got = _engine_results(name)
    assert sorted("ref:" + k for k in got) == sorted(k for k in rec if k.startswith("ref:"))
    errs = {k: fr.rel_l2(t, rec["ref:" + k]) for k, t in got.items()}
    print(name, {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(t.dtype == torch.float32 for t in got.values())
    assert all(tuple(t.shape) == rec["ref:" + k].shape for k, t in got.items())
    assert all(e <= 1e-5 for e in errs.values()), errs


@needs_reference
@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_live_reference_helper_and_fixtures_agree(name):
    grid, L, ratio = fr.CASES[name]
    dim = len(grid)
    rec = dict(np.load(os.path.join(fr.GOLDEN, name + ".npz")))
    ref = fr.load_reference_differentiation()
    u, v = _leaves(rec, torch.float64)
    with fr.default_float64():
        live = fr.run_all(ref.FourierDiff(dim, L=L if dim > 1 else L[0], low_pass_filter_ratio=ratio), u, v,
                          int(rec["gseed"]), dim)
    u, v = _leaves(rec, torch.float64)
    helper = fr.run_all(fr.F64FourierDiff(dim, L, ratio), u, v, int(rec["gseed"]), dim)
    _, got = _engine_results(name)
    for k, t in live.items():
        assert fr.rel_l2(t, rec["ref:" + k]) <= 1e-12, k               # the fixtures are what the reference computes
        assert fr.rel_l2(helper[k], t) <= 1e-12, k
        assert fr.rel_l2(got[k], t) <= 1e-5, k


@needs_reference
def test_live_reference_in_fp32_with_default_L():
    """the reference as its users run it (fp32 input, fp32 frequencies, L = 2 pi) against the engine"""
    ref = fr.load_reference_differentiation()
    g = torch.Generator().manual_seed(9)
    u = torch.randn(3, 10, 12, generator=g)
    want = ref.FourierDiff(2).gradient(u)
    with engine_on_emulation():
        got = FourierDiff(2).gradient(u)
    assert fr.rel_l2(got, want) <= 1e-5


def test_double_backward_and_input_dtypes():
    """d/du of |grad_u <lap u, c>|^2: the backward pass is the operator itself, so autograd differentiates it again;
    float64 / bfloat16 input is computed and returned in fp32"""
    g = torch.Generator().manual_seed(4)
    u = torch.randn(2, 7, 6, generator=g).requires_grad_(True)
    c = torch.randn(2, 7, 6, generator=g).requires_grad_(True)
    with engine_on_emulation():
        fd = FourierDiff(2, L=(1.3, 0.7))
        gu, = torch.autograd.grad((fd.laplacian(u) * c).sum(), u, create_graph=True)
        gc, = torch.autograd.grad(gu.square().sum(), c)
        out64 = fd.dx(u.detach().double())
        out16 = fd.dx(u.detach().bfloat16())
        base = fd.dx(u.detach())
        wide = fd.dx(u.detach().bfloat16().float())
    h = fr.F64FourierDiff(2, (1.3, 0.7))
    u64, c64 = u.detach().double().requires_grad_(True), c.detach().double().requires_grad_(True)
    gu64, = torch.autograd.grad((h.laplacian(u64) * c64).sum(), u64, create_graph=True)
    gc64, = torch.autograd.grad(gu64.square().sum(), c64)
    assert fr.rel_l2(gu.detach(), gu64.detach()) <= 1e-5 and fr.rel_l2(gc, gc64) <= 1e-5
    assert out64.dtype == out16.dtype == torch.float32
    assert torch.equal(out64, base) and torch.equal(out16, wide)


def test_error_paths_raise_what_the_reference_raises():
    with pytest.raises(ValueError, match="dim must be 1, 2, or 3"):
        FourierDiff(4)
    with pytest.raises(ValueError, match="L must be a single float or tuple with 2 elements"):
        FourierDiff(2, L=(1.0, 2.0, 3.0))
    with pytest.raises(NotImplementedError, match="Fourier continuation"):
        FourierDiff(2, use_fc="Legendre")
    with pytest.raises(NotImplementedError, match="Fourier continuation"):
        FourierDiff(1, use_fc="gram")
    with pytest.raises(ValueError, match="not valid"):
        FourierDiff(1, use_fc="chebyshev")
    u1, u2 = torch.zeros(2, 8), torch.zeros(2, 2, 8, 8)
    f1, f2, f3 = FourierDiff(1), FourierDiff(2), FourierDiff(3)
    assert f1.L == 2 * torch.pi and f2.L == (2 * torch.pi,) * 2
    with pytest.raises(ValueError, match="dy method only available"):
        f1.dy(u1)
    with pytest.raises(ValueError, match="dz method only available"):
        f2.dz(u2)
    with pytest.raises(ValueError, match="curl not defined for 1D"):
        f1.curl(u1)
    with pytest.raises(ValueError, match="Invalid direction 'y' for dimension 1"):
        f1.partial(u1, direction="y")
    with pytest.raises(ValueError, match="order must be a tuple with 2 elements"):
        f2.derivative(u2, (1,))
    with pytest.raises(ValueError, match="input must have 2 components"):
        f2.divergence(torch.zeros(3, 8, 8))
    with pytest.raises(ValueError, match="For 2D, input must have 2 components"):
        f2.curl(torch.zeros(3, 8, 8))
    with pytest.raises(ValueError, match="For 3D, input must have 3 components"):
        f3.curl(torch.zeros(2, 4, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU path"):
        f2.dx(u2)                                              # the product has no host fall-back
