"""gloo tests (CPU) of the skip-path resample of the spatially decomposed ("pencil") layer,
``SpatialParallelSpectralConv.transform``: the halo-row exchange (mpu.mappings.exchange_rows) and the 2-d bicubic
stage, and the distributed spectral resample of 3-d grids, against the single-process resample of the gathered
tensor.  The local stages are torch stand-ins (tests/pencil_resample_ops.py); tests/test_spatial_resample_emu.py
runs the engine's own kernels instead."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


def _worker(rank, world, port, spatial, out_shape, rsf, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    from neuraloperator_amd import SpectralConv
    from neuraloperator_amd.mpu import SpatialParallelSpectralConv, comm
    from pencil_resample_ops import PencilResampleOps, spectral_resample

    comm.init(model_parallel_size=world, backend="gloo")
    nd = len(spatial)
    modes = (4,) * nd
    conv = SpatialParallelSpectralConv(3, 3, modes, ops=PencilResampleOps(), resolution_scaling_factor=rsf)
    torch.manual_seed(0)                      # identical full tensors on every rank
    x = torch.randn(2, 3, *spatial)
    if rsf is not None:
        og = [round(n * f) for n, f in zip(spatial, [rsf] * nd if not isinstance(rsf, list) else rsf)]
    else:
        og = list(out_shape)
    g = torch.randn(2, 3, *og)
    hl, ho = spatial[0] // world, og[0] // world
    xs = x[:, :, rank * hl:(rank + 1) * hl].clone().requires_grad_(True)
    y = conv.transform(xs, output_shape=out_shape)
    assert list(y.shape) == [2, 3, ho, *og[1:]], y.shape
    y.backward(g[:, :, rank * ho:(rank + 1) * ho])

    xf = x.clone().requires_grad_(True)
    if nd == 2:                               # the single-GPU layer's skip path (ATen's interpolator on CPU)
        yf = SpectralConv(3, 3, modes).transform(xf, output_shape=og)
    else:                                     # (its 3-d path runs on the engine: resample.py:54-66 restated)
        yf = spectral_resample(xf, og)
    yf.backward(g)
    ret[rank] = dict(y=_rel(y, yf[:, :, rank * ho:(rank + 1) * ho]),
                     gx=_rel(xs.grad, xf.grad[:, :, rank * hl:(rank + 1) * hl]))
    comm.cleanup()


def _run(world, spatial, out_shape, rsf, tol):
    from neuraloperator_amd.mpu import comm
    port = comm.free_port()
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, spatial, out_shape, rsf, ret), nprocs=world, join=True)
    assert len(ret) == world
    for rank, errs in ret.items():
        for k, v in errs.items():
            assert v <= tol, (rank, k, v)


CASES_2D = [((32, 24), (48, 40), None),        # up
            ((64, 48), (32, 20), None),        # down
            ((32, 24), None, [1.5, 0.75]),     # resolution_scaling_factor (non-square output)
            ((40, 16), (24, 36), None)]        # non-square, down along rows / up along columns


@pytest.mark.parametrize("world", [2, 4, 8])
@pytest.mark.parametrize("spatial,out_shape,rsf", CASES_2D)
def test_bicubic_skip_path_on_row_shards(world, spatial, out_shape, rsf):
    _run(world, spatial, out_shape, rsf, 1e-6)


def test_bicubic_one_input_row_per_rank():
    """8 rows over 8 ranks -> 16: an output row's taps reach two ranks away"""
    _run(8, (8, 6), (16, 10), None, 1e-6)


@pytest.mark.parametrize("world", [2, 4, 8])
@pytest.mark.parametrize("spatial,out_shape", [((8, 8, 6), (16, 8, 6)), ((16, 8, 6), (8, 12, 10))])
def test_spectral_skip_path_on_row_shards(world, spatial, out_shape):
    _run(world, spatial, out_shape, None, 1e-5)


def test_no_resolution_change_returns_the_input():
    from neuraloperator_amd.mpu import SpatialParallelSpectralConv
    from pencil_resample_ops import PencilResampleOps
    conv = SpatialParallelSpectralConv(2, 2, (4, 4), ops=PencilResampleOps())
    x = torch.randn(1, 2, 8, 6)
    assert conv.transform(x) is x
    assert conv.transform(x, output_shape=(8, 6)) is x


def test_complex_data_skip_path_is_out_of_scope():
    from neuraloperator_amd.mpu import SpatialParallelSpectralConv
    from pencil_resample_ops import PencilResampleOps
    conv = SpatialParallelSpectralConv(2, 2, (4, 4), ops=PencilResampleOps(), complex_data=True)
    with pytest.raises(NotImplementedError, match="complex_data"):
        conv.transform(torch.randn(1, 2, 8, 6, dtype=torch.cfloat), output_shape=(16, 6))
