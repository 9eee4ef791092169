"""CPU tier: the finite-difference convolution kernels (sc_kernels_fdconv.h) in host emulation through the C-ABI against
the float64 helper (tests/fdconv_reference.py): forward, data gradient and weight gradient of both routes, the route a
descriptor takes, refusals, bit-identical repeats.  The emulation runs one OS thread per lane: case-table sizes only."""
import ctypes

import pytest
import torch

import fdconv_reference as fr
from emu_engine import engine_on_emulation
from neuraloperator_amd import _lib


@pytest.fixture(scope="module")
def emu():
    with engine_on_emulation() as lib:
        yield lib


_desc, _run = fr.desc_of, fr.run_descriptor             # the runner the GPU tier drives on the device


ALL_CASES = {**fr.CASES, **fr.LIVE_CASES}


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_both_routes_against_the_float64_helper(emu, name):
    cfg = ALL_CASES[name]
    x, w, g = fr.case_inputs(cfg, 77)
    h = fr.grid_width_of(cfg)
    assert emu.fdconv_path(_desc(cfg, h)) == cfg["route"]
    y, gx, gw = _run(emu, cfg, x, w, g, h)
    want = [t.numpy() for t in fr.fdconv_with_grads(x, w, g, h, cfg["groups"], cfg["padding"])]
    scales = fr.magnitudes(x, w, g, h, cfg["groups"], cfg["padding"])
    # where the stencil cancels (smooth field): twice the error of the reference's own formula in fp32 on the same input
    bars = fr.smooth_bars(x, w, g, h, cfg["groups"], cfg["padding"], want) if cfg["smooth"] else (1e-5, 1e-5, 1e-5)
    errs = fr.check_against(cfg, (y.numpy(), gx.numpy(), gw.numpy()), want, bars, scales)
    if cfg["smooth"]:
        print(name, "ratio to the fp32 formula's own error", " ".join(f"{2 * e / b:.2f}" for e, b in zip(errs, bars)))
    print(name, " ".join(f"{e:.1e}" for e in errs))
    assert not gw.numpy()[fr.centre_index(cfg)].any()


@pytest.mark.parametrize("name", fr.EMU_KERNEL_CASES)
def test_kernel_edge_cases_small_enough_for_the_emulation(emu, name):
    """the cases of tests/test_gpu_fdconv_kernels.py that finish here in seconds, at that file's two bars: rel-L2 1e-5
    per tensor and |got - want| <= gamma_N A per element (fdconv_reference.abs_bounds)"""
    cfg = fr.KERNEL_CASES[name]
    x, w, g = fr.case_inputs(cfg, 91)
    h = fr.grid_width_of(cfg)
    assert emu.fdconv_path(_desc(cfg, h)) == cfg["route"]
    got = [t.numpy() for t in _run(emu, cfg, x, w, g, h)]
    want = [t.numpy() for t in fr.fdconv_with_grads(x, w, g, h, cfg["groups"], cfg["padding"])]
    fr.check_against(cfg, got, want, (1e-5, 1e-5, 1e-5), fr.magnitudes(x, w, g, h, cfg["groups"], cfg["padding"]))
    bounds, ns = fr.abs_bounds(cfg, x, w, g, h)
    ratios = [fr.worst_ratio(a, b, A, n) for a, b, A, n in zip(got, want, bounds, ns)]
    print(name, "worst |err| / (gamma_N A)", " ".join(f"{r:.3f}" for r in ratios))
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("name", ["2d_k3_replicate_g2", "2d_mfma_zeros_32_b1", "3d_k3_reflect"])
def test_repeats_are_bit_identical_and_one_gradient_alone_is_the_same(emu, name):
    cfg = fr.CASES[name]
    x, w, g = fr.case_inputs(cfg, 78)
    h = fr.grid_width_of(cfg)
    a, b = _run(emu, cfg, x, w, g, h), _run(emu, cfg, x, w, g, h)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    _, gx, none = _run(emu, cfg, x, w, g, h, want_w=False)
    assert none is None and torch.equal(gx, a[1])
    _, none, gw = _run(emu, cfg, x, w, g, h, want_x=False)
    assert none is None and torch.equal(gw, a[2])


def test_route_of_a_descriptor(emu):
    D = _lib.ScEngineLib.fdconv_desc
    for ci in (32, 64, 128):
        for co in (32, 64, 128):
            for pad in ("periodic", "zeros"):
                assert emu.fdconv_path(D(dims=(8, 8), batch=1, c_in=ci, c_out=co, k=3, padding=pad)) == fr.MFMA
    good = dict(dims=(8, 8), batch=1, c_in=32, c_out=32, k=3)
    for other in (dict(k=5), dict(groups=2), dict(c_in=33), dict(c_out=96), dict(padding="reflect"),
                  dict(padding="replicate"), dict(dims=(8,)), dict(dims=(4, 8, 8))):
        assert emu.fdconv_path(D(**{**good, **other})) == fr.GENERAL, other


def test_refusals_before_any_launch(emu):
    L, D = emu.lib, _lib.ScEngineLib.fdconv_desc
    buf = torch.zeros(1 << 16)
    p, n = buf.data_ptr(), buf.numel() * 4
    good = dict(dims=(6, 6), batch=1, c_in=4, c_out=4, k=3)
    bad = [dict(k=4), dict(k=2), dict(k=9), dict(k=1), dict(groups=3), dict(c_in=6, c_out=4, groups=3),
           dict(padding="reflect", dims=(6, 1)), dict(padding="reflect", k=5, dims=(2, 6)),
           dict(padding="periodic", k=7, dims=(2, 6)), dict(dims=(6, 0)), dict(dims=()), dict(dims=(2, 2, 2, 2)),
           dict(batch=0), dict(c_in=0), dict(padding=7), dict(groups=0), dict(inv_h=float("nan"))]
    for change in bad:
        d = D(**{**good, **change})
        assert L.sc_fdconv_path(ctypes.byref(d)) == 0, change
        assert L.sc_fdconv_workspace_bytes(ctypes.byref(d)) == 0, change
        assert L.sc_fdconv_forward(ctypes.byref(d), p, p, p, p, n, None) != 0, change
        assert "sc_engine" in L.sc_last_error().decode()
        assert L.sc_fdconv_backward(ctypes.byref(d), p, p, p, p, p, p, n, None) != 0, change
    d = D(**good)
    ok = ctypes.byref(d)
    assert L.sc_fdconv_path(None) == 0 and L.sc_fdconv_workspace_bytes(None) == 0
    assert L.sc_fdconv_forward(None, p, p, p, p, n, None) != 0
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.sc_fdconv_forward(ok, *args, n, None) != 0
    assert L.sc_fdconv_forward(ok, p, p, p, p, 8, None) != 0                    # workspace too small
    for args in ((p, p, None, p, p, p), (p, p, p, None, None, p), (p, p, p, p, p, None), (None, p, p, p, p, p),
                 (p, None, p, p, p, p)):
        assert L.sc_fdconv_backward(ok, *args, n, None) != 0
    assert L.sc_fdconv_backward(ok, p, p, p, p, p, p, 8, None) != 0
    assert float(buf.abs().sum()) == 0.0                                        # no refused call wrote anything
    # valid calls with one gradient, each tensor in a buffer of its own
    cfg = fr._case((6, 6), 4, 4, batch=1)
    x, w, g = fr.case_inputs(cfg, 5)
    ws, gx, gw = torch.zeros(1 << 12), torch.full_like(x, float("nan")), torch.full_like(w, float("nan"))
    nb = ws.numel() * 4
    assert nb >= L.sc_fdconv_workspace_bytes(ok) >= L.sc_fdconv_forward_workspace_bytes(ok) > 0
    assert L.sc_fdconv_backward(ok, None, w.data_ptr(), g.data_ptr(), gx.data_ptr(), None, ws.data_ptr(), nb, None) == 0
    assert L.sc_fdconv_backward(ok, x.data_ptr(), None, g.data_ptr(), None, gw.data_ptr(), ws.data_ptr(), nb, None) == 0
    want = fr.fdconv_with_grads(x, w, g, 1.0, 1, "periodic")     # x is not needed for gx alone, nor the weight for gw alone
    assert fr.rel_l2(gx.numpy(), want[1].numpy()) <= 1e-5 and fr.rel_l2(gw.numpy(), want[2].numpy()) <= 1e-5
