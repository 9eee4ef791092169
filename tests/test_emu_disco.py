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


def _cfg(in_shape, support, c_in=3, c_out=5, stride=(1, 1), padding=None, opad=(0, 0), groups=1, basis=4, batch=2,
         transposed=False, bias=True, route=dr.GENERAL):
    padding = tuple((p + 1) // 2 - 1 for p in support) if padding is None else padding
    return dict(in_shape=in_shape, support=support, c_in=c_in, c_out=c_out, stride=stride, padding=padding, opad=opad,
                groups=groups, basis=basis, batch=batch, transposed=transposed, bias=bias, route=route)


CASES = {
    "3x3_one_past_a_tile_column": _cfg((5, 65), (3, 3)),
    "3x3_one_past_a_tile_row": _cfg((17, 6), (3, 3), batch=1),
    "5x5_stride2": _cfg((18, 21), (5, 5), stride=(2, 2)),
    "7x5_strides_3x4_pad_small": _cfg((20, 23), (7, 5), stride=(3, 4), padding=(1, 0), batch=1),
    "4x3_even_rectangular": _cfg((9, 10), (4, 3)),
    "2x2_pad0": _cfg((7, 7), (2, 2)),
    "15x15_cap": _cfg((17, 16), (15, 15), c_in=2, c_out=2, batch=1),
    "1x1": _cfg((4, 5), (1, 1)),
    "groups2_odd_channels": _cfg((6, 7), (3, 3), c_in=6, c_out=10, groups=2),
    "depthwise_one_row": _cfg((1, 9), (3, 3), c_in=5, c_out=5, groups=5),
    "no_bias_stride4": _cfg((16, 12), (5, 9), stride=(4, 4), bias=False, batch=1),
    "transpose_stride2": _cfg((5, 6), (5, 5), stride=(2, 2), opad=(1, 1), transposed=True),
    "transpose_strides_2x3_grouped": _cfg((4, 5), (7, 5), c_in=4, c_out=6, stride=(2, 3), opad=(1, 0), groups=2,
                                          transposed=True),
    "transpose_stride1_even": _cfg((6, 6), (4, 4), padding=(2, 2), transposed=True, batch=1),
    "transpose_past_a_tile": _cfg((9, 33), (3, 3), stride=(2, 2), opad=(1, 1), c_in=2, c_out=3, batch=1,
                                  transposed=True),
    "mfma_32_32": _cfg((5, 34), (3, 3), c_in=32, c_out=32, batch=1, route=dr.MFMA),
    "mfma_64_32_no_bias": _cfg((4, 8), (3, 3), c_in=64, c_out=32, batch=1, bias=False, route=dr.MFMA),
    "mfma_32_64_transposed": _cfg((4, 8), (3, 3), c_in=32, c_out=64, batch=2, transposed=True, route=dr.MFMA),
}


def _weight_shape(cfg):
    if cfg["transposed"]:
        return (cfg["c_in"], cfg["c_out"] // cfg["groups"], cfg["basis"])
    return (cfg["c_out"], cfg["c_in"] // cfg["groups"], cfg["basis"])


def _inputs(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    x = dr.fp32_randn((cfg["batch"], cfg["c_in"], *cfg["in_shape"]), g)
    w = dr.fp32_randn(_weight_shape(cfg), g) * 0.3
    psi = dr.fp32_randn((cfg["basis"], *cfg["support"]), g)
    b = dr.fp32_randn((cfg["c_out"],), g) if cfg["bias"] else None
    shape = dr.out_shape_of(x.shape, cfg["c_out"], psi.shape, cfg["stride"], cfg["padding"], cfg["opad"],
                            cfg["transposed"])
    return x, w, psi, b, dr.fp32_randn(shape, g)


Q = 0.0625


def _desc(cfg, out_shape, **over):
    kw = dict(batch=cfg["batch"], c_in=cfg["c_in"], c_out=cfg["c_out"], in_shape=cfg["in_shape"], out_shape=out_shape,
              basis=cfg["basis"], support=cfg["support"], stride=cfg["stride"], padding=cfg["padding"],
              output_padding=cfg["opad"], groups=cfg["groups"], q_weight=Q, transposed=cfg["transposed"])
    kw.update(over)
    return _lib.ScEngineLib.disco_desc(**kw)


def _run(lib, cfg, x, w, psi, b, g, want=(True, True, True)):
    """sc_disco_forward + sc_disco_backward on host tensors: (out, gx, gw, gbias)"""
    d = _desc(cfg, g.shape[2:])
    nbytes, fbytes = lib.disco_workspace_bytes(d), lib.disco_forward_workspace_bytes(d)
    assert 0 < fbytes <= nbytes
    ws = torch.empty(nbytes, dtype=torch.uint8)
    y = torch.full(tuple(g.shape), float("nan"))
    lib.disco_forward(d, x.data_ptr(), w.data_ptr(), psi.data_ptr(), 0 if b is None else b.data_ptr(), y.data_ptr(),
                      ws.data_ptr(), fbytes)                 # its own, smaller size
    gx = torch.full_like(x, float("nan")) if want[0] else None
    gw = torch.full_like(w, float("nan")) if want[1] else None
    gb = torch.full((cfg["c_out"],), float("nan")) if want[2] else None
    ws.fill_(0xff)                                           # the backward call owes nothing to the forward call's workspace
    lib.disco_backward(d, x.data_ptr(), w.data_ptr(), psi.data_ptr(), g.data_ptr(), *(0 if t is None else t.data_ptr()
                                                                                        for t in (gx, gw, gb)),
                       ws.data_ptr(), nbytes)
    return y, gx, gw, gb


def _want(cfg, x, w, psi, b, g):
    out, gx, gw, gb = dr.disco_with_grads(x, w, b, psi, g, Q, cfg["stride"], cfg["padding"], cfg["opad"], cfg["groups"],
                                          cfg["transposed"])
    if gb is None:                                           # the bias gradient does not need a bias
        gb = g.double().sum(dim=(0, 2, 3))
    return out, gx, gw, gb


@pytest.mark.parametrize("name", sorted(CASES))
def test_both_routes_against_the_float64_helper(emu, name):
    cfg = CASES[name]
    x, w, psi, b, g = _inputs(cfg, 91)
    assert emu.disco_path(_desc(cfg, g.shape[2:])) == cfg["route"]
    got = _run(emu, cfg, x, w, psi, b, g)
    errs = [dr.rel_l2(a.numpy(), t.numpy()) for a, t in zip(got, _want(cfg, x, w, psi, b, g))]
    print(name, " ".join(f"{e:.1e}" for e in errs))
    assert max(errs) <= 1e-5, errs


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
