"""GPU tier: the complex32 wire and fno_block_precision "half" / "mixed" on the distributed layers, on the MI355X.

* k_wire_pack_c32 / k_wire_unpack_c32 against torch's float32 <-> float16 casts on the device, bit for bit (a NaN as a
  NaN), at the per-rank shapes of BASELINE configs[3] on 8 ranks and at ragged / windowed small shapes;
* a one-rank RCCL group: ModeParallelSpectralConv and SpatialParallelSpectralConv at "half" / "mixed" against
  SpectralConv(fno_block_precision=p) on the same device and against the half_2d / mixed_2d / mixed_3d goldens under
  the single-GPU rule (tests/test_emu_half.py); the mode-parallel step's four exchanges go over the complex32 wire."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from engine_runner import rel_l2

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _values(numel, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(numel, generator=g) * 10.0 ** torch.randint(-9, 6, (numel,), generator=g).float()
    special = torch.tensor([0.0, -0.0, 65504.0, 65519.9, 65520.0, -65520.0, 1e9, 5.96e-8, 2.98e-8, 2.99e-8, 6.1e-5,
                            6.09e-5, float("inf"), float("-inf"), float("nan")])
    ties = 1.0 + torch.arange(64).float() * 2.0 ** -11 + 2.0 ** -12
    extra = torch.cat([special, ties])[:numel]
    v[torch.randperm(numel, generator=g)[:extra.numel()]] = extra
    return v


def _spec(shape, seed):
    return torch.view_as_complex(_values(int(np.prod(shape)) * 2, seed).reshape(*shape, 2)).to(DEV)


def _pack_ref(spec, P, rows, w0):
    n, c, k1 = spec.shape[:3]
    full = torch.zeros(n, c, P * rows, *spec.shape[3:], dtype=torch.complex64, device=spec.device)
    full[:, :, w0:w0 + k1] = spec
    wire = full.reshape(n, c, P, rows, *spec.shape[3:]).movedim(2, 0)
    return torch.view_as_real(wire).half().contiguous().view(torch.int32).squeeze(-1)


def _unpack_ref(wire, k1, w0):
    P, n, c, rows = wire.shape[:4]
    halves = wire.contiguous().unsqueeze(-1).view(torch.float16)
    full = torch.view_as_complex(halves.float().contiguous()).movedim(0, 2).reshape(n, c, P * rows, *wire.shape[4:])
    return full[:, :, w0:w0 + k1]


def _same_words(a, b):
    """complex32 words bit for bit; a NaN half only as a NaN"""
    ha, hb = a.contiguous().view(torch.int16).int() & 0xffff, b.contiguous().view(torch.int16).int() & 0xffff
    nan = ((hb & 0x7c00) == 0x7c00) & ((hb & 0x3ff) != 0)
    nan_a = ((ha & 0x7c00) == 0x7c00) & ((ha & 0x3ff) != 0)
    return torch.equal(nan, nan_a) and torch.equal(ha[~nan], hb[~nan])


def _same_c64(a, b):
    ra, rb = torch.view_as_real(a).contiguous(), torch.view_as_real(b).contiguous()
    nan = torch.isnan(rb)
    return torch.equal(torch.isnan(ra), nan) and torch.equal(ra.view(torch.int32)[~nan], rb.view(torch.int32)[~nan])


# (spectrum shape (n, C, k1, *rest), P, rows, w0); configs[3] on 8 ranks: one sample per rank, 32 channels, kept block
# 32 x 32 x 17, 4 of the 32 first-dim rows per rank
CASES = [
    ((1, 32, 32, 32, 17), 8, 4, 0),        # way out: this rank's xhat -> the send wire
    ((8, 32, 4, 32, 17), 1, 4, 0),         # way back: the contraction's result -> the send wire (plain conversion)
    ((2, 3, 5, 7), 3, 2, 0),               # ragged: rank 2 carries one zero row; odd rows
    ((1, 2, 6, 4, 5), 8, 4, 13),           # a window across rank boundaries
    ((3, 4, 9, 6), 8, 2, 0),               # ranks 5..7 carry zero rows only
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{'x'.join(map(str, c[0]))}_P{c[1]}_rows{c[2]}_w{c[3]}")
def test_wire_kernels_are_torchs_cast_on_the_device(case):
    from neuraloperator_amd import engine
    shape, P, rows, w0 = case
    spec = _spec(shape, seed=sum(shape) + P)
    wire = engine.wire_pack_c32(spec, P, rows, w0)
    torch.cuda.synchronize()
    assert _same_words(wire, _pack_ref(spec, P, rows, w0))
    # the inverse gather of the same window, and the whole wire as a plain conversion
    back = engine.wire_unpack_c32(wire, shape[2], w0)
    torch.cuda.synchronize()
    assert _same_c64(back, _unpack_ref(wire, shape[2], w0))
    whole = engine.wire_unpack_c32(wire.view(1, -1, *wire.shape[2:]), rows, 0)
    assert _same_c64(whole, _unpack_ref(wire.view(1, -1, *wire.shape[2:]), rows, 0))


def test_wire_unpack_of_every_float16_pattern_on_the_device():
    from neuraloperator_amd import engine
    h = torch.arange(1 << 16, dtype=torch.int32).to(torch.int16)              # every pattern, NaNs included
    wire = h.view(torch.int32).reshape(1, 1, 1, 1, -1).to(DEV)
    got = engine.wire_unpack_c32(wire, 1, 0)
    ref = torch.view_as_complex(wire.view(torch.float16).float().reshape(1, 1, 1, -1, 2))
    assert _same_c64(got, ref)


# ---- one-rank RCCL group: the distributed layers at half / mixed -------------------------------------------------
@pytest.fixture
def one_rank_group():
    from neuraloperator_amd.mpu import comm
    port = comm.free_port()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    comm.init(model_parallel_size=1, backend="nccl")
    try:
        yield
    finally:
        comm.cleanup()


def _golden_rule(y, ref, bias, gx, gw, gb, g):
    """tests/test_emu_half.py's rule against the reference's float16 arithmetic"""
    yb, rb = y - bias, ref - bias
    step = torch.maximum(rb.abs(), torch.tensor(6.1e-5)) * 2.0 ** -10
    assert bool(((yb - rb).abs() <= 1.01 * step).all())
    assert ((yb - rb).abs() <= 1e-7).float().mean().item() > 0.98
    assert rel_l2(gx, g["gx"]) < 2e-3
    if gw is not None:
        assert rel_l2(gw, g["gw"]) < 2e-3
    assert rel_l2(gb, g["gbias"]) < 1e-5


def _single_gpu(g, x, gy):
    from neuraloperator_amd import SpectralConv
    ci, co = g["w"].shape[:2]
    conv = SpectralConv(ci, co, tuple(int(v) for v in g["ctor_n_modes"]), fno_block_precision=str(g["precision"])).to(DEV)
    with torch.no_grad():
        conv.weight.tensor.copy_(torch.from_numpy(g["w"]))
        conv.bias.copy_(torch.from_numpy(g["bias"]))
    xd = x.to(DEV, copy=True).requires_grad_(True)
    y = conv(xd)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    return y.detach().cpu(), xd.grad.cpu(), conv.weight.tensor.grad.cpu(), conv.bias.grad.cpu()


@pytest.mark.parametrize("name", ["half_2d", "mixed_2d", "mixed_3d"])
def test_mode_parallel_half_on_a_one_rank_rccl_group(one_rank_group, name):
    from neuraloperator_amd.mpu import ModeParallelSpectralConv
    from neuraloperator_amd.mpu.mappings import A2A_STATS
    g = load_golden(name)
    x, gy = torch.from_numpy(g["x"]), torch.from_numpy(g["g"])
    ci, co = g["w"].shape[:2]
    layer = ModeParallelSpectralConv(ci, co, tuple(int(v) for v in g["ctor_n_modes"]),
                                     fno_block_precision=str(g["precision"])).to(DEV)
    layer.load_full_state_dict({"weight.tensor": torch.from_numpy(g["w"]), "bias": torch.from_numpy(g["bias"])})
    xd = x.to(DEV, copy=True).requires_grad_(True)
    A2A_STATS["bytes"], A2A_STATS["calls"] = 0, 0
    y = layer(xd)
    y.backward(gy.to(DEV))
    layer.reduce_replicated_grads()
    torch.cuda.synchronize()
    # four exchanges on the complex32 wire: 4 bytes per mode of xhat, yhat, g_yhat, g_xhat
    modes = layer.rows * int(np.prod(layer.max_n_modes[1:]))
    assert A2A_STATS["calls"] == 4
    assert A2A_STATS["bytes"] == 4 * 2 * x.shape[0] * (ci + co) * modes
    y, gx, gw, gb = y.detach().cpu(), xd.grad.cpu(), layer.weight.grad.cpu(), layer.bias.grad.cpu()
    # the single-GPU layer on the same device: the same stages, the same bits
    ys, gxs, gws, gbs = _single_gpu(g, x, gy)
    assert (y == ys).float().mean().item() >= 0.999
    assert rel_l2(gx.numpy(), gxs.numpy()) <= 1e-5
    assert rel_l2(torch.view_as_real(gw).numpy(), torch.view_as_real(gws).numpy()) <= 1e-5
    assert rel_l2(gb.numpy(), gbs.numpy()) <= 1e-5
    _golden_rule(y, torch.from_numpy(g["y"]), torch.from_numpy(g["bias"]), gx.numpy(), gw.numpy(), gb.numpy(), g)


@pytest.mark.parametrize("name", ["half_2d", "mixed_2d", "mixed_3d"])
def test_pencil_half_on_a_one_rank_rccl_group(one_rank_group, name):
    from neuraloperator_amd.mpu import SpatialParallelSpectralConv
    g = load_golden(name)
    x, gy = torch.from_numpy(g["x"]), torch.from_numpy(g["g"])
    ci, co = g["w"].shape[:2]
    layer = SpatialParallelSpectralConv(ci, co, tuple(int(v) for v in g["ctor_n_modes"]),
                                        fno_block_precision=str(g["precision"])).to(DEV)
    with torch.no_grad():
        layer.weight.copy_(SpatialParallelSpectralConv.shard_dense_weight(torch.from_numpy(g["w"]), 0, 1).to(DEV))
        layer.bias.copy_(torch.from_numpy(g["bias"]).reshape(layer.bias.shape))
    xd = x.to(DEV, copy=True).requires_grad_(True)
    y = layer(xd)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    y, gx, gb = y.detach().cpu(), xd.grad.cpu(), layer.bias.grad.cpu()
    k2 = g["w"].shape[3]
    gw = layer.weight.grad.cpu()[:, :, :, :k2]
    # the single-GPU layer: the same cast points; the separable transform differs in the last fp32 bits
    ys, gxs, gws, gbs = _single_gpu(g, x, gy)
    bias = torch.from_numpy(g["bias"])
    step = torch.maximum((ys - bias).abs(), torch.tensor(6.1e-5)) * 2.0 ** -10
    assert bool(((y - ys).abs() <= 1.01 * step).all())
    assert rel_l2(gx.numpy(), gxs.numpy()) < 2e-3
    assert rel_l2(torch.view_as_real(gw).numpy(), torch.view_as_real(gws).numpy()) < 2e-3
    _golden_rule(y, torch.from_numpy(g["y"]), bias, gx.numpy(), gw.numpy(), gb.numpy(), g)
