"""GPU tier: the skip-path resample of the spatially decomposed layer on the MI355X.

1. The bicubic row-range kernels (sc_bicubic_rows_forward / _backward) on row shards of ONE device: for P ranks each
   shard's halo'd rows (mpu.spatial_parallel.bicubic_source_rows) are sliced out of a full tensor, run through the
   entry points and the pieces put back together -- against F.interpolate(bicubic, align_corners=True) and its autograd
   gradient on the same device.  The gather-form backward is deterministic.
2. ``SpatialParallelSpectralConv.transform`` at P = 1 (no process group) against ``SpectralConv.transform``: 2-d
   through the new kernels (the route is asserted), 3-d through the engine's spectral resample."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


def _sharded(x, g, out_grid, P):
    """the per-rank kernel calls of a P-way row decomposition, pieces gathered (the gradient's halo rows summed)"""
    from neuraloperator_amd import _lib
    from neuraloperator_amd.mpu.spatial_parallel import bicubic_source_rows
    lib = _lib.get_lib()
    n, h, w = x.shape
    ho, wo = out_grid
    hp = ho // P
    ys, gx, gx_again = [], torch.zeros_like(x), torch.zeros_like(x)
    for p, (lo, hi) in enumerate(bicubic_source_rows(h, ho, P)):
        xs = x[:, lo:hi].contiguous()
        gs = g[:, p * hp:(p + 1) * hp].contiguous()
        y = torch.empty(n, hp, wo, device=x.device)
        lib.bicubic_rows_forward(xs.data_ptr(), y.data_ptr(), n, hi - lo, w, lo, h, ho, wo, p * hp, hp)
        ys.append(y)
        for acc in (gx, gx_again):
            gp = torch.empty_like(xs)
            lib.bicubic_rows_backward(gs.data_ptr(), gp.data_ptr(), n, hi - lo, w, lo, h, ho, wo, p * hp, hp)
            acc[:, lo:hi] += gp
    torch.cuda.synchronize()
    return torch.cat(ys, 1), gx, gx_again


@pytest.mark.parametrize("P", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("n,grid,out_grid", [(6, (32, 24), (48, 40)),       # up
                                             (6, (64, 48), (24, 20)),       # down
                                             (5, (33, 19), (24, 27)),       # odd sizes, rows down / columns up
                                             (3, (45, 31), (72, 17))])      # odd sizes, rows up / columns down
def test_bicubic_row_kernels_on_emulated_shards(P, n, grid, out_grid):
    dev = torch.device("cuda:0")
    torch.manual_seed(P)
    x = torch.randn(n, *grid, device=dev)
    xr = x[:, None].clone().requires_grad_(True)
    ref = F.interpolate(xr, size=out_grid, mode="bicubic", align_corners=True)
    g = torch.randn_like(ref)
    ref.backward(g)
    y, gx, gx_again = _sharded(x, g[:, 0].contiguous(), out_grid, P)
    assert _rel(y, ref[:, 0]) <= 1e-6
    assert _rel(gx, xr.grad[:, 0]) <= 1e-6
    assert torch.equal(gx, gx_again)


@pytest.mark.parametrize("P", [1, 2, 4, 8])
@pytest.mark.parametrize("grid,out_grid", [((1024, 1024), (2048, 2048)), ((2048, 2048), (1024, 1024))])
def test_bicubic_row_kernels_user_scale(P, grid, out_grid):
    """B * C = 64 at 1024^2 <-> 2048^2"""
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.randn(64, *grid, device=dev)
    xr = x[:, None].clone().requires_grad_(True)
    ref = F.interpolate(xr, size=out_grid, mode="bicubic", align_corners=True)
    g = torch.randn_like(ref)
    ref.backward(g)
    y, gx, gx_again = _sharded(x, g[:, 0].contiguous(), out_grid, P)
    assert _rel(y, ref[:, 0]) <= 1e-6
    assert _rel(gx, xr.grad[:, 0]) <= 1e-6
    assert torch.equal(gx, gx_again)


@pytest.mark.parametrize("spatial,out_shape,rsf,tol", [((32, 24), (48, 40), None, 1e-6),
                                                       ((64, 48), None, [0.5, 0.75], 1e-6),
                                                       ((12, 16, 20), (24, 16, 10), None, 1e-5),
                                                       ((16, 8, 6), (8, 12, 10), None, 1e-5)])
def test_pencil_transform_on_device_single_rank(spatial, out_shape, rsf, tol, monkeypatch):
    from neuraloperator_amd import SpectralConv, _lib
    from neuraloperator_amd.mpu import SpatialParallelSpectralConv

    dev = torch.device("cuda:0")
    nd = len(spatial)
    calls = []
    lib = _lib.get_lib()
    for name in ("bicubic_rows_forward", "bicubic_rows_backward"):
        fn = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _fn=fn, _name=name, **k: (calls.append(_name), _fn(*a, **k))[1])
    sp = SpatialParallelSpectralConv(4, 4, (4,) * nd, resolution_scaling_factor=rsf).to(dev)
    ref = SpectralConv(4, 4, (4,) * nd, resolution_scaling_factor=rsf).to(dev)
    assert sp.P == 1
    torch.manual_seed(2)
    x = torch.randn(2, 4, *spatial, device=dev)
    xs, xf = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y = sp.transform(xs, output_shape=out_shape)
    yf = ref.transform(xf, output_shape=out_shape)
    assert y.shape == yf.shape
    g = torch.randn_like(yf)
    y.backward(g)
    yf.backward(g)
    assert _rel(y, yf) <= tol
    assert _rel(xs.grad, xf.grad) <= tol
    if nd == 2:
        assert calls == ["bicubic_rows_forward", "bicubic_rows_backward"]
    else:
        assert calls == []
