"""GPU tier: the equidistant discrete-continuous convolutions on an MI355X -- every recorded fixture at the bar of
tests/test_disco_reference.py, layers at the smallest shapes that cross a tile, stride, support-cap or route edge
against the float64 helper on the host, the route each takes, bit-identical repeats, and one forward + backward step of
a layer and of a LocalNOBlocks layer replayed from a captured graph.

Shapes: with domain_length = the fine grid's shape the grid spacing is 1 and the support is floor(2 radius_cutoff) + 1
per axis, whatever the extents (3 x 3 for the default cutoff at stride 1, 5 x 5 at stride 2, 7 x 7 at stride 3)."""
import pytest
import torch

import disco_reference as dr
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _path(m, x):
    from neuraloperator_amd import _lib, engine
    pad, opad = m._geometry()
    d = engine.DiscoConvFn.desc(x, m.weight, m.get_local_filter_matrix(), m.groups, (m.scale_h, m.scale_w), pad, opad,
                                m.q_weight, m._transposed)
    return _lib.get_lib().disco_path(d)


@pytest.mark.parametrize("name", sorted(dr.CASES))
def test_layer_matches_the_recorded_reference(name):
    cfg, rec = dr.CASES[name], load_golden("disco_" + name)
    m, out, gx, gw, gb = dr.run_module(cfg, rec, DEV)
    assert tuple(out.shape) == tuple(int(v) for v in rec["out_shape"])
    errs = {"out": dr.rel_l2(out, rec["out"]), "grad:x": dr.rel_l2(gx, rec["grad:x"]),
            "grad:weight": dr.rel_l2(gw, rec["grad:weight"])}
    if gb is not None:
        errs["grad:bias"] = dr.rel_l2(gb, rec["grad:bias"])
    print(name, " ".join(f"{k}={e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= 1e-5, (k, e)


def _unit(in_shape, out_shape, c_in, c_out, transposed=False, route=dr.GENERAL, batch=1, support=None, **kw):
    fine = out_shape if transposed else in_shape
    kw.setdefault("domain_length", [float(fine[0]), float(fine[1])])
    return dict(kwargs=dict(in_channels=c_in, out_channels=c_out, in_shape=in_shape, out_shape=out_shape,
                            kernel_shape=[2, 4], **kw), batch=batch, transposed=transposed, route=route, support=support)


HELPER_CASES = {
    "one_past_a_tile_17x65": _unit((17, 65), (17, 65), 3, 5, support=(3, 3)),
    "stride2_34x130_to_17x65": _unit((34, 130), (17, 65), 3, 5, support=(5, 5)),
    "cap_15x15": _unit((33, 33), (33, 33), 2, 3, radius_cutoff=0.45, domain_length=[2, 2], support=(15, 15)),
    "odd_channels_33_31": _unit((9, 20), (9, 20), 33, 31, support=(3, 3)),
    "depthwise_one_row": _unit((1, 70), (1, 70), 8, 8, groups=8, support=(3, 3)),
    "mfma_32_32_4x36": _unit((4, 36), (4, 36), 32, 32, route=dr.MFMA, batch=2, support=(3, 3)),
    "mfma_64_128_16x16": _unit((16, 16), (16, 16), 64, 128, route=dr.MFMA, domain_length=[2, 2], support=(3, 3)),
    "mfma_128_32_8x40": _unit((8, 40), (8, 40), 128, 32, route=dr.MFMA, support=(3, 3)),
    "transpose_9x33_to_18x99": _unit((9, 33), (18, 99), 3, 4, transposed=True, support=(7, 7)),
}


def _build(cfg, seed):
    """the layer of a helper case with random bias, its inputs, and the float64 helper's results on the host"""
    torch.manual_seed(seed)
    m = dr.own_class(cfg["transposed"])(**cfg["kwargs"])
    assert (m.psi_local_h, m.psi_local_w) == cfg["support"]
    x, w, b = dr.case_inputs(cfg, m, seed)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    stride, pad, opad = dr.geometry(m.psi_local_h, m.psi_local_w, m.scale_h, m.scale_w, cfg["transposed"])
    psi = m.get_local_filter_matrix()
    shape = dr.out_shape_of(x.shape, cfg["kwargs"]["out_channels"], psi.shape, stride, pad, opad, cfg["transposed"])
    g = dr.cotangent(shape, seed)
    return m, x, g, (stride, pad, opad, psi)


def _run(m, x, g):
    m = m.to(DEV)
    m.zero_grad(set_to_none=True)
    xd = x.to(DEV).requires_grad_(True)
    assert m.on_engine(xd)
    out = m(xd)
    out.backward(g.to(DEV))
    return out.detach().cpu(), xd.grad.cpu(), m.weight.grad.cpu(), m.bias.grad.cpu()


@pytest.mark.parametrize("name", sorted(HELPER_CASES))
def test_edge_shapes_against_the_float64_helper(name):
    cfg = HELPER_CASES[name]
    m, x, g, (stride, pad, opad, psi) = _build(cfg, 91)
    want = dr.disco_with_grads(x, m.weight, m.bias, psi, g, m.q_weight, stride, pad, opad, m.groups, cfg["transposed"])
    assert _path(m, x) == cfg["route"]
    got = _run(m, x, g)
    errs = [dr.rel_l2(a.numpy(), t.numpy()) for a, t in zip(got, want)]
    print(name, " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 1e-5, errs


@pytest.mark.parametrize("name", ["stride2_34x130_to_17x65", "mfma_32_32_4x36", "transpose_9x33_to_18x99"])
def test_repeats_are_bit_identical(name):
    m, x, g, _ = _build(HELPER_CASES[name], 92)
    a, b = _run(m, x, g), _run(m, x, g)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def _graph_equals_eager(module, call, x0, gout, fresh):
    """captures one forward + backward step of `module` and replays it on new inputs: equal to eager, bit for bit"""
    params = [p for p in module.parameters()]

    def eager(xv):
        xv = xv.detach().clone().requires_grad_(True)
        module.zero_grad(set_to_none=True)
        out = call(xv)
        out.backward(gout)
        return [out.detach().clone(), xv.grad.clone()] + [p.grad.clone() for p in params]

    x = x0.clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                               # warm-up off the capture, on a leaf of its own
        warm = x0.clone().requires_grad_(True)
        for _ in range(2):
            call(warm).backward(gout)
    torch.cuda.current_stream().wait_stream(s)
    module.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(x)
        out.backward(gout)
    static = [p.grad for p in params]
    for new in fresh:
        with torch.no_grad():
            x.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        got = [out.detach().clone(), x.grad.clone()] + [t.clone() for t in static]
        want = eager(new)
        for p, t in zip(params, static):
            p.grad = t
        assert all(torch.equal(u, v) for u, v in zip(got, want))


@pytest.mark.parametrize("name", ["stride2_34x130_to_17x65", "mfma_32_32_4x36"])
def test_layer_step_replays_from_a_captured_graph(name):
    m, x, g, _ = _build(HELPER_CASES[name], 93)
    m = m.to(DEV)
    gen = torch.Generator().manual_seed(94)
    fresh = [torch.randn(x.shape, generator=gen).to(DEV) for _ in range(2)]
    _graph_equals_eager(m, m, x.to(DEV), g.to(DEV), fresh)


def test_local_no_block_step_replays_from_a_captured_graph():
    from neuraloperator_amd import LocalNOBlocks
    torch.manual_seed(95)
    blocks = LocalNOBlocks(32, 32, (8, 8), (16, 16), n_layers=2).to(DEV)
    gen = torch.Generator().manual_seed(96)
    x, g = torch.randn(2, 32, 16, 16, generator=gen).to(DEV), torch.randn(2, 32, 16, 16, generator=gen).to(DEV)
    fresh = [torch.randn(2, 32, 16, 16, generator=gen).to(DEV) for _ in range(2)]
    layer0 = [p for k, p in blocks.named_parameters() if ".0." in k]

    class Layer0(torch.nn.Module):                           # the parameters layer 0 uses, so that every one has a gradient
        def __init__(self):
            super().__init__()
            self.ps = torch.nn.ParameterList(layer0)

        def forward(self, v):
            return blocks(v, 0)

    step = Layer0()
    assert _path(blocks.local_convs[0], x) == dr.MFMA
    _graph_equals_eager(step, step, x, g, fresh)
