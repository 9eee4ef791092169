"""CPU tier: the discrete-continuous convolution kernels (sc_kernels_disco.h) in host emulation through the C-ABI against
the float64 helper (tests/disco_reference.py): forward, data gradient, weight gradient and bias gradient of both routes
and both forms, the route a descriptor takes, refusals before any launch, bit-identical repeats.  The descriptors here
are free-standing (a random basis buffer, any support / stride / padding the entry points accept), not only those a
layer builds.  The emulation runs one OS thread per lane: small extents only."""
import ctypes

import pytest
import torch

import disco_reference as dr
from emu_engine import engine_on_emulation
from neuraloperator_amd import _lib


@pytest.fixture(scope="module")
def emu():
    with engine_on_emulation() as lib:
        yield lib


# the descriptor runners and the case list live in disco_reference.py: the GPU tier drives them on the device
_cfg, _inputs, _desc, _run, _want = dr.desc_case, dr.desc_inputs, dr.desc_of, dr.run_descriptor, dr.desc_want
CASES, Q = dr.DESC_CASES, dr.Q


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_routes_against_the_float64_helper(emu, name):
    cfg = CASES[name]
    x, w, psi, b, g = _inputs(cfg, 91)
    assert emu.disco_path(_desc(cfg, g.shape[2:])) == cfg["route"]
    got = _run(emu, cfg, x, w, psi, b, g)
    errs = [dr.rel_l2(a.numpy(), t.numpy()) for a, t in zip(got, _want(cfg, x, w, psi, b, g))]
    print(name, " ".join(f"{e:.1e}" for e in errs))
    assert max(errs) <= 1e-5, errs


@pytest.mark.parametrize("name", dr.EMU_KERNEL_CASES)
def test_kernel_edge_cases_small_enough_for_the_emulation(emu, name):
    """the cases of tests/test_gpu_disco_kernels.py that finish here in seconds, at that file's two bars: rel-L2 1e-5
    per tensor and |got - want| <= gamma_N A per element (disco_reference.abs_bounds)"""
    cfg = dr.KERNEL_CASES[name]
    x, w, psi, b, g = _inputs(cfg, 91)
    assert emu.disco_path(_desc(cfg, g.shape[2:])) == cfg["route"]
    got = [t.numpy() for t in _run(emu, cfg, x, w, psi, b, g)]
    want = [t.numpy() for t in _want(cfg, x, w, psi, b, g)]
    errs = [dr.rel_l2(a, t) for a, t in zip(got, want)]
    assert max(errs) <= 1e-5, errs
    bounds, ns = dr.abs_bounds(cfg, x, w, psi, b, g)
    ratios = [dr.worst_ratio(a, t, A.numpy(), n) for a, t, A, n in zip(got, want, bounds, ns)]
    print(name, "worst |err| / (gamma_N A)", " ".join(f"{r:.3f}" for r in ratios))
    assert max(ratios) <= 1.0, ratios


@pytest.mark.parametrize("name", ["5x5_stride2", "transpose_strides_2x3_grouped", "mfma_32_32"])
def test_repeats_are_bit_identical_and_one_gradient_alone_is_the_same(emu, name):
    cfg = CASES[name]
    x, w, psi, b, g = _inputs(cfg, 92)
    a, c = _run(emu, cfg, x, w, psi, b, g), _run(emu, cfg, x, w, psi, b, g)
    assert all(torch.equal(u, v) for u, v in zip(a, c))
    for i in range(3):
        want = tuple(j == i for j in range(3))
        one = _run(emu, cfg, x, w, psi, b, g, want)
        assert torch.equal(one[1 + i], a[1 + i]) and sum(t is not None for t in one[1:]) == 1


def test_route_of_a_descriptor(emu):
    D = _lib.ScEngineLib.disco_desc
    good = dict(batch=1, in_shape=(8, 8), out_shape=(8, 8), basis=5, support=(3, 3), padding=(1, 1))
    for ci in (32, 64, 128):
        for co in (32, 64, 128):
            for tr in (False, True):
                assert emu.disco_path(D(c_in=ci, c_out=co, transposed=tr, **good)) == dr.MFMA
    base = dict(c_in=32, c_out=32, **good)
    others = (dict(groups=2), dict(c_in=33), dict(c_out=96), dict(support=(3, 5), padding=(1, 2)),
              dict(support=(2, 2), padding=(0, 0), out_shape=(7, 7)), dict(padding=(0, 0), out_shape=(6, 6)),
              dict(in_shape=(16, 16), stride=(2, 2), support=(3, 3), out_shape=(8, 8)))
    for other in others:
        assert emu.disco_path(D(**{**base, **other})) == dr.GENERAL, other


def test_refusals_before_any_launch(emu):
    L, D = emu.lib, _lib.ScEngineLib.disco_desc
    buf = torch.zeros(1 << 16)
    p, n = buf.data_ptr(), buf.numel() * 4
    good = dict(batch=1, c_in=4, c_out=4, in_shape=(6, 6), out_shape=(6, 6), basis=5, support=(3, 3), padding=(1, 1))
    bad = [dict(out_shape=(6, 5)), dict(out_shape=(7, 6)), dict(out_shape=(0, 6)),      # extents that do not follow
           dict(stride=(2, 2)),                                                        # ... (3, 3) would
           dict(groups=3), dict(c_in=6, groups=3), dict(groups=0),
           dict(support=(16, 3), padding=(7, 1), out_shape=(5, 6)), dict(support=(0, 3)),  # support beyond the cap
           dict(stride=(5, 1), out_shape=(2, 6)), dict(stride=(1, 0)),                  # stride beyond the cap
           dict(padding=(3, 1), out_shape=(10, 6)), dict(padding=(-1, 1), out_shape=(4, 6)),
           dict(output_padding=(1, 0)),                                                 # belongs to the transposed form
           dict(transposed=True, output_padding=(1, 0), out_shape=(7, 6)),              # not below the stride
           dict(transposed=True, out_shape=(6, 7)), dict(transposed=2),
           dict(batch=0), dict(c_out=0), dict(basis=0), dict(q_weight=float("nan")), dict(q_weight=float("inf")),
           dict(in_shape=(6, 1 << 30), out_shape=(6, 1 << 30)),                         # offsets beyond the index types
           dict(batch=1 << 28, in_shape=(1 << 12, 1 << 12), out_shape=(1 << 12, 1 << 12)),
           dict(support=(7, 7), padding=(0, 0), out_shape=(0, 0))]                      # support larger than the input
    for change in bad:
        d = D(**{**good, **change})
        assert L.sc_disco_path(ctypes.byref(d)) == 0, change
        assert L.sc_disco_workspace_bytes(ctypes.byref(d)) == 0 == L.sc_disco_forward_workspace_bytes(ctypes.byref(d))
        assert L.sc_disco_forward(ctypes.byref(d), p, p, p, p, p, p, n, None) != 0, change
        assert "sc_engine" in L.sc_last_error().decode()
        assert L.sc_disco_backward(ctypes.byref(d), p, p, p, p, p, p, p, p, n, None) != 0, change
    d = D(**good)
    ok = ctypes.byref(d)
    assert L.sc_disco_path(None) == 0 and L.sc_disco_workspace_bytes(None) == 0
    assert L.sc_disco_forward(None, p, p, p, p, p, p, n, None) != 0
    for args in ((None, p, p, p, p, p), (p, None, p, p, p, p), (p, p, None, p, p, p), (p, p, p, p, None, p),
                 (p, p, p, p, p, None)):
        assert L.sc_disco_forward(ok, *args, n, None) != 0, args
    assert L.sc_disco_forward(ok, p, p, p, p, p, p, 8, None) != 0               # workspace too small
    #                 x  w  psi gout gx gw gb ws
    for args in ((p, p, p, None, p, p, p, p), (p, p, p, p, None, None, None, p), (p, p, p, p, p, p, p, None),
                 (None, p, p, p, None, p, None, p), (p, None, p, p, p, None, None, p), (p, p, None, p, p, None, None, p),
                 (p, p, None, p, None, p, None, p)):
        assert L.sc_disco_backward(ok, *args, n, None) != 0, args
    assert L.sc_disco_backward(ok, p, p, p, p, p, p, p, p, 8, None) != 0
    assert float(buf.abs().sum()) == 0.0                                        # no refused call wrote anything
    # valid calls with one gradient and only the tensors it needs; the bias gradient alone needs no workspace
    cfg = _cfg((6, 6), (3, 3), c_in=4, c_out=4, basis=5, batch=1)
    x, w, psi, b, g = _inputs(cfg, 5)
    want = _want(cfg, x, w, psi, b, g)
    ws, gx, gw, gb = torch.zeros(1 << 12), torch.full_like(x, float("nan")), torch.full_like(w, float("nan")), \
        torch.full((4,), float("nan"))
    nb = ws.numel() * 4
    dd = ctypes.byref(_desc(cfg, (6, 6)))
    assert nb >= L.sc_disco_workspace_bytes(dd) >= L.sc_disco_forward_workspace_bytes(dd) > 0
    assert L.sc_disco_backward(dd, None, w.data_ptr(), psi.data_ptr(), g.data_ptr(), gx.data_ptr(), None, None,
                               ws.data_ptr(), nb, None) == 0
    assert L.sc_disco_backward(dd, x.data_ptr(), None, psi.data_ptr(), g.data_ptr(), None, gw.data_ptr(), None,
                               ws.data_ptr(), nb, None) == 0
    assert L.sc_disco_backward(dd, None, None, None, g.data_ptr(), None, None, gb.data_ptr(), None, 0, None) == 0
    for a, t in zip((gx, gw, gb), want[1:]):
        assert dr.rel_l2(a.numpy(), t.numpy()) <= 1e-5
