"""GPU tier of ``neuraloperator_amd.FiniteDiff`` / ``LpLoss`` / ``H1Loss`` (sc_kernels_stencil.h): every fixture recorded
from the verbatim reference classes (tests/golden/finite_diff_*.npz, sobolev_loss_*.npz), forward and backward, at 1e-5;
shapes the small fixtures cannot reach -- several chunks per line, ragged rows, more rows than a tile, one line over the
whole device -- against the float64 helper (tests/finite_diff_reference.py), periodic and with one axis non-periodic;
bit-identical repeat launches; one H1Loss step under hipGraph capture."""
import os

import numpy as np
import pytest
import torch

import finite_diff_reference as fdr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def test_the_three_names_import():
    from neuraloperator_amd import FiniteDiff, H1Loss, LpLoss
    assert FiniteDiff(2).h == (1.0, 1.0) and H1Loss(d=2).name == "H1_2DLoss" and LpLoss(d=3).name == "L2_3Dloss"


def _rec(name):
    return dict(np.load(os.path.join(fdr.GOLDEN, name + ".npz")))


def _scalar_err(a, b):
    a, b = float(a), float(b)
    return abs(a - b) / abs(b) if b != 0 else abs(a)


@pytest.mark.parametrize("name", sorted(fdr.CASES))
def test_finite_diff_fixtures_forward_and_backward_on_device(name):
    from neuraloperator_amd import FiniteDiff
    grid, h, periodic = fdr.CASES[name]
    dim = len(grid)
    rec = _rec(name)
    u = torch.from_numpy(rec["u"]).to(DEV).requires_grad_(True)
    v = torch.from_numpy(rec["v"]).to(DEV).requires_grad_(True)
    fd = FiniteDiff(dim, h=h if dim > 1 else h[0], **{"periodic_in_" + "xyz"[a]: periodic[a] for a in range(dim)})
    got = fdr.run_all(fd, u, v, int(rec["gseed"]), dim)
    torch.cuda.synchronize()
    errs = {k: fdr.rel_l2(t.cpu(), rec["ref:" + k]) for k, t in got.items()}
    print(name, {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(e <= 1e-5 for e in errs.values()), errs


@pytest.mark.parametrize("name", sorted(fdr.LOSS_CASES))
def test_loss_fixtures_value_and_gradient_on_device(name):
    from neuraloperator_amd import H1Loss, LpLoss
    rec = _rec(name)
    x = torch.from_numpy(rec["x"]).to(DEV).requires_grad_(True)
    y = torch.from_numpy(rec["y"]).to(DEV)
    got = fdr.run_losses({"LpLoss": LpLoss, "H1Loss": H1Loss}, x, y, name)
    torch.cuda.synchronize()
    errs = {k: (fdr.rel_l2(t.cpu(), rec["ref:" + k]) if k.endswith(":grad") else _scalar_err(t.cpu(), rec["ref:" + k]))
            for k, t in got.items()}
    print(name, {k: f"{e:.2e}" for k, e in errs.items()})
    assert all(t.dtype == torch.float32 for t in got.values())
    assert all(e <= 1e-5 for e in errs.values()), {k: e for k, e in errs.items() if e > 1e-5}


# operand shape, spatial dims
SHAPES = [((3, 2, 70, 130), 2),        # several chunks per line, ragged rows, three row tiles
          ((2, 2, 6, 10, 67), 3),
          ((33, 4100), 1),
          ((1, 1, 256, 256), 2)]       # one line over the whole device
_HOST = {}


def _host_case(shape, d, variant):
    """operands, float64 helper results and gradients: computed once per (shape, variant), shared, left unchanged"""
    key = (shape, variant)
    if key not in _HOST:
        g = torch.Generator().manual_seed(sum(shape))
        x, y = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
        periodic = tuple(not (variant == "np" and a == d - 1 - (d > 1)) for a in range(d))   # the second-to-last axis
        h = tuple(0.5 + 0.25 * a for a in range(d))
        hf = fdr.F64FiniteDiff(d, h, periodic)
        cot = torch.randn(*shape, generator=g, dtype=torch.float64)
        want = {}
        x64 = x.double().requires_grad_(True)
        for m in ("laplacian", "dx"):
            out = getattr(hf, m)(x64)
            gr, = torch.autograd.grad((out * cot).sum(), x64)
            want[m] = (out.detach(), gr)
        for k, kw in (("h1", dict(h1=True, periodic=periodic)), ("lp2", dict(p=2)), ("lp1", dict(p=1))):
            val = fdr.f64_loss(x64, y.double(), d, "rel", measure=[1.0 + 0.5 * a for a in range(d)], **kw)
            gr, = torch.autograd.grad(val, x64)
            want[k] = (val.detach(), gr)
        _HOST[key] = (x, y, periodic, h, cot, want)
    return _HOST[key]


@pytest.mark.parametrize("variant", ["per", "np"])
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s[0])) for s in SHAPES])
def test_larger_shapes_against_the_float64_helper(shape, variant):
    from neuraloperator_amd import FiniteDiff, H1Loss, LpLoss
    dims, d = shape
    x, y, periodic, h, cot, want = _host_case(dims, d, variant)
    flags = {"periodic_in_" + "xyz"[a]: periodic[a] for a in range(d)}
    measure = [1.0 + 0.5 * a for a in range(d)]
    fd = FiniteDiff(d, h=h if d > 1 else h[0], **flags)
    errs = {}
    for m in ("laplacian", "dx"):
        xd = x.to(DEV).requires_grad_(True)
        out = getattr(fd, m)(xd)
        gr, = torch.autograd.grad((out * cot.float().to(DEV)).sum(), xd)
        errs[m] = (fdr.rel_l2(out.detach().cpu(), want[m][0]), fdr.rel_l2(gr.cpu(), want[m][1]))
    for k, loss in (("h1", H1Loss(d=d, measure=measure, **flags)), ("lp2", LpLoss(d=d, p=2, measure=measure)),
                    ("lp1", LpLoss(d=d, p=1, measure=measure))):
        xd = x.to(DEV).requires_grad_(True)
        val = loss(xd, y.to(DEV))
        gr, = torch.autograd.grad(val, xd)
        errs[k] = (_scalar_err(val.cpu(), want[k][0]), fdr.rel_l2(gr.cpu(), want[k][1]))
    torch.cuda.synchronize()
    print(dims, variant, {k: [f"{e:.2e}" for e in v] for k, v in errs.items()})
    assert all(max(v) <= 1e-5 for v in errs.values()), errs


def test_two_launches_are_bit_identical():
    from neuraloperator_amd import FiniteDiff, H1Loss, LpLoss
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(3, 2, 70, 130, generator=g).to(DEV), torch.randn(3, 2, 70, 130, generator=g).to(DEV)
    fd, h1, lp = FiniteDiff(2, h=(1.0, 2.0), periodic_in_y=False), H1Loss(d=2, periodic_in_x=False), LpLoss(d=2, p=3)
    runs = []
    for _ in range(2):
        xi = x.clone().requires_grad_(True)
        lap = fd.laplacian(xi)
        a, b = h1(xi, y), lp(xi, y)
        (a + b + lap.square().sum()).backward()
        torch.cuda.synchronize()
        runs.append((lap.detach().cpu(), a.detach().cpu(), b.detach().cpu(), xi.grad.cpu()))
    for p, q in zip(*runs):
        assert torch.equal(p, q)


def test_h1_step_under_graph_capture_replayed_with_changed_inputs():
    from neuraloperator_amd import H1Loss
    g = torch.Generator().manual_seed(6)
    data = [(torch.randn(4, 2, 40, 70, generator=g), torch.randn(4, 2, 40, 70, generator=g)) for _ in range(3)]
    loss_fn = H1Loss(d=2, periodic_in_y=False)
    x = data[0][0].to(DEV).requires_grad_(True)
    y = data[0][1].to(DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):                        # the tables are built outside the capture
        for _ in range(2):
            x.grad = None
            loss_fn(x, y).backward()
    torch.cuda.current_stream(DEV).wait_stream(side)
    x.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                        # linear: two launches forward, one backward; the workspace
        loss = loss_fn(x, y)                             # comes from torch's allocator inside the capture
        loss.backward()
    for xn, yn in data[1:]:
        with torch.no_grad():
            x.copy_(xn.to(DEV))
            y.copy_(yn.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        xe = xn.to(DEV).requires_grad_(True)
        le = loss_fn(xe, yn.to(DEV))
        le.backward()
        torch.cuda.synchronize()
        assert torch.equal(loss.detach(), le.detach()) and torch.equal(x.grad, xe.grad)


def test_host_input_is_refused():
    from neuraloperator_amd import FiniteDiff, H1Loss
    with pytest.raises(RuntimeError, match="no CPU path"):
        FiniteDiff(2).dx(torch.zeros(2, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        H1Loss(d=2)(torch.zeros(2, 8, 8), torch.ones(2, 8, 8))
