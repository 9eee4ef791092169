"""GPU tier of ``neuraloperator_amd.FourierDiff`` (sc_kernels_specop.h between a full-spectrum transform pair): every
fixture recorded from the verbatim reference class (tests/golden/fourier_diff_*.npz), forward and backward, at 1e-5;
shapes the small fixtures cannot reach against the float64 helper (tests/fourier_diff_reference.py); gradient ->
divergence = laplacian on odd grids; bit-identical repeat launches; one step under hipGraph capture."""
import os

import numpy as np
import pytest
import torch

import fourier_diff_reference as fr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_fixtures_forward_and_backward_on_device(name):
    from neuraloperator_amd import FourierDiff
    grid, L, ratio = fr.CASES[name]
    dim = len(grid)
    rec = dict(np.load(os.path.join(fr.GOLDEN, name + ".npz")))
    u = torch.from_numpy(rec["u"]).to(DEV).requires_grad_(True)
    v = torch.from_numpy(rec["v"]).to(DEV).requires_grad_(True)
    fd = FourierDiff(dim, L=L if dim > 1 else L[0], low_pass_filter_ratio=ratio)
    got = fr.run_all(fd, u, v, int(rec["gseed"]), dim)
    torch.cuda.synchronize()
    errs = {k: fr.rel_l2(t.cpu(), rec["ref:" + k]) for k, t in got.items()}
    print(name, {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(e <= 1e-5 for e in errs.values()), errs


def _check(fd, h, method, x, lim=1e-5):
    """method of the engine class on the device against the float64 helper, output and gradient"""
    g = torch.Generator().manual_seed(31)
    xd = x.to(DEV).requires_grad_(True)
    y = getattr(fd, method)(xd)
    cot = torch.randn(y.shape, generator=g)
    y.backward(cot.to(DEV))
    torch.cuda.synchronize()
    x64 = x.double().requires_grad_(True)
    y64 = getattr(h, method)(x64)
    y64.backward(cot.double())
    errs = (fr.rel_l2(y.detach().cpu(), y64.detach()), fr.rel_l2(xd.grad.cpu(), x64.grad))
    print(method, tuple(x.shape), [f"{e:.2e}" for e in errs])
    assert max(errs) <= lim, (method, errs)


# leading + spatial shape, dim, L, ratio, methods
SHAPES = [((3, 16, 256), 2, (1.3, 2.9), None, ("gradient", "laplacian")),     # kept 16 x 129: odd rows, both lane widths
          ((2, 2, 64, 66), 2, (2.0, 0.7), 0.75, ("gradient", "laplacian")),    # kept 64 x 34
          ((33, 12, 10), 2, (1.0, 1.0), None, ("gradient", "laplacian")),      # many groups, tiny rows
          ((2, 8, 12, 20), 3, (1.5, 0.9, 2.6), None, ("gradient", "laplacian")),
          ((4096, 64), 1, (3.3,), None, ("gradient", "laplacian")),            # many lines
          ((2, 5, 8, 600), 2, (1.0, 2.0), None, ("gradient",))]                # kept 8 x 301: waves side by side


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s[0])) for s in SHAPES])
def test_larger_shapes_against_the_float64_helper(shape):
    from neuraloperator_amd import FourierDiff
    dims, dim, L, ratio, methods = shape
    g = torch.Generator().manual_seed(sum(dims))
    x = torch.randn(*dims, generator=g)
    fd = FourierDiff(dim, L=L if dim > 1 else L[0], low_pass_filter_ratio=ratio)
    h = fr.F64FourierDiff(dim, L, ratio)
    for m in methods:
        _check(fd, h, m, x)


def test_vector_operators_3d_three_sources_six_terms():
    from neuraloperator_amd import FourierDiff
    g = torch.Generator().manual_seed(8)
    v = torch.randn(2, 3, 8, 12, 20, generator=g)
    L = (1.5, 0.9, 2.6)
    fd, h = FourierDiff(3, L=L), fr.F64FourierDiff(3, L)
    _check(fd, h, "curl", v)
    _check(fd, h, "divergence", v)
    many = [(1, 0, 2), (0, 0, 0), (2, 1, 0), (0, 3, 1), (1, 1, 1), (0, 0, 2), (2, 0, 0), (0, 2, 0), (3, 0, 1)]
    u = v[:, 0].contiguous()
    got = fd.compute_multiple_derivatives(u.to(DEV), many)
    want = h.compute_multiple_derivatives(u, many)
    assert len(got) == 9 and all(fr.rel_l2(a.cpu(), b) <= 1e-5 for a, b in zip(got, want))


@pytest.mark.parametrize("grid", [(15, 21), (7, 9, 11)], ids=["15x21", "7x9x11"])
def test_divergence_of_gradient_is_the_laplacian_on_odd_grids(grid):
    """no Nyquist plane on an odd grid: (i k)^1 (i k)^1 = (i k)^2 mode by mode"""
    from neuraloperator_amd import FourierDiff
    g = torch.Generator().manual_seed(12)
    u = torch.randn(3, *grid, generator=g).to(DEV)
    fd = FourierDiff(len(grid), L=tuple(1.0 + 0.5 * d for d in range(len(grid))))
    lap, div = fd.laplacian(u), fd.divergence(fd.gradient(u))
    assert fr.rel_l2(div.cpu(), lap.cpu()) <= 1e-5


def test_two_launches_are_bit_identical():
    from neuraloperator_amd import FourierDiff
    g = torch.Generator().manual_seed(3)
    v = torch.randn(4, 2, 64, 130, generator=g).to(DEV)
    fd = FourierDiff(2, L=(1.0, 2.0))
    runs = []
    for _ in range(2):
        vi = v.clone().requires_grad_(True)
        c = fd.curl(vi)
        gr = fd.gradient(c)
        gr.square().sum().backward()
        torch.cuda.synchronize()
        runs.append((c.detach().cpu(), gr.detach().cpu(), vi.grad.cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_one_step_under_graph_capture():
    from neuraloperator_amd import FourierDiff, capture_step

    class Lap(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fd = FourierDiff(2, L=(1.0, 2.0))

        def forward(self, x):
            return self.fd.laplacian(x)

    g = torch.Generator().manual_seed(6)
    x0, x1 = torch.randn(4, 32, 34, generator=g), torch.randn(4, 32, 34, generator=g)
    go = torch.randn(4, 32, 34, generator=g).to(DEV)
    mod = Lap()
    x = x0.to(DEV).requires_grad_(True)
    step = capture_step(mod, x, go)
    with torch.no_grad():
        x.copy_(x1.to(DEV))
    y = step.replay()
    torch.cuda.synchronize()
    xe = x1.to(DEV).requires_grad_(True)
    ye = mod(xe)
    ye.backward(go)
    torch.cuda.synchronize()
    assert torch.equal(y, ye.detach()) and torch.equal(x.grad, xe.grad)


def test_host_input_is_refused():
    from neuraloperator_amd import FourierDiff
    with pytest.raises(RuntimeError, match="no CPU path"):
        FourierDiff(2).dx(torch.zeros(2, 8, 8))
