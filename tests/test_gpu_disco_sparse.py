"""GPU tier: the point-cloud discrete-continuous convolutions on an MI355X -- every recorded fixture at the bar of
tests/test_disco_sparse_reference.py, the descriptor list of the emulation tier through the C-ABI on the device, layers
at channel counts and point counts that cross a lane chunk, a row tile and a slice of the weight gradient against the
float64 helper on the host, one larger cloud, the route each takes, bit-identical repeats, and one forward + backward
step of a layer replayed from a captured graph."""
import pytest
import torch

import disco_sparse_reference as ds
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("name", sorted(ds.CASES))
def test_layer_matches_the_recorded_reference(name):
    cfg, rec = ds.CASES[name], load_golden("dsparse_" + name)
    m = ds.own_class(cfg["transposed"])(grid_in=torch.from_numpy(rec["grid_in"]), grid_out=torch.from_numpy(rec["grid_out"]),
                                        quadrature_weights=torch.from_numpy(rec["q"]), **cfg["kwargs"]).to(DEV)
    assert m.on_engine(torch.from_numpy(rec["x"]).to(DEV)) == (not cfg["float64"])
    out, gx, gw, gb = ds.run_module(m, rec, DEV)
    errs = {"out": ds.rel_l2(out, rec["out"]), "grad:x": ds.rel_l2(gx, rec["grad:x"]),
            "grad:weight": ds.rel_l2(gw, rec["grad:weight"])}
    if gb is not None:
        errs["grad:bias"] = ds.rel_l2(gb, rec["grad:bias"])
    print(name, " ".join(f"{k}={e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= 1e-5, (k, e)
    if cfg["lonely"]:                                        # no neighbour: the bias alone
        assert (out[:, :, ds.LONELY] == rec["bias"][None, :]).all()


@pytest.mark.parametrize("name", sorted(ds.DESC_CASES))
def test_descriptors_against_the_float64_helper(name):
    from neuraloperator_amd import _lib
    cfg = ds.DESC_CASES[name]
    psi, keep, x, w, q, b, g = ds.desc_inputs(cfg, 91)
    got = ds.run_descriptor(_lib.get_lib(), cfg, psi, keep, x, w, q, b, g, device=DEV, stream=_stream())
    want = ds.sparse_disco_with_grads(x, w, b, psi.double(), q, g, cfg["groups"])
    errs = [ds.rel_l2(a.numpy(), t.numpy()) if float(t.abs().max()) > 0 else float(a.abs().max())
            for a, t in zip(got[:4], want)]
    print(name, " ".join(f"{e:.1e}" for e in errs))
    assert max(errs) <= 1e-5, errs
    for o, k in cfg["empty"]:
        assert float(got[4][o, :, k].abs().max()) == 0.0


def _layer(n_in, n_out, c_in, c_out, batch=2, transposed=False, route=ds.GENERAL, **kw):
    return dict(kwargs=dict(in_channels=c_in, out_channels=c_out, kernel_shape=[2, 4], **kw), n_in=n_in, n_out=n_out,
                batch=batch, transposed=transposed, float64=False, lonely=False, route=route)


# a layer's Psi at these sizes: 20 to 40 entries to a row, a few rows empty
LAYER_CASES = {
    "odd_channels_33_31": _layer(300, 129, 33, 31, batch=1),
    "batch_times_channels_65": _layer(200, 100, 13, 4, batch=5),
    "groups4_of_8": _layer(257, 129, 32, 24, groups=4),
    "depthwise_16": _layer(257, 129, 16, 16, groups=16),
    "transpose_130_to_300": _layer(130, 300, 6, 10, transposed=True),
    "larger_cloud_5000_to_3000": _layer(5000, 3000, 8, 8),
    "mfma_32_32": _layer(257, 129, 32, 32, route=ds.MFMA),
    "mfma_64_128_transposed": _layer(130, 300, 64, 128, batch=1, transposed=True, route=ds.MFMA),
    "mfma_128_32": _layer(200, 65, 128, 32, batch=3, route=ds.MFMA),
}


def _build(cfg, seed):
    torch.manual_seed(seed)
    m = ds.build_own(cfg, seed)
    x, w, b, g = ds.case_inputs(cfg, m, seed)
    with torch.no_grad():
        m.weight.copy_(w)
        m.bias.copy_(b)
    return m, x, g


def _run(m, x, g):
    m = m.to(DEV)
    m.zero_grad(set_to_none=True)
    xd = x.to(DEV).requires_grad_(True)
    assert m.on_engine(xd)
    out = m(xd)
    out.backward(g.to(DEV))
    return out.detach().cpu(), xd.grad.cpu(), m.weight.grad.cpu(), m.bias.grad.cpu()


def _path(m, x):
    from neuraloperator_amd import _lib, engine
    return _lib.get_lib().dsparse_path(engine.SparseDiscoFn.desc(x, m.weight, m.n_out, m.csr_vals.numel(), m.groups))


@pytest.mark.parametrize("name", sorted(LAYER_CASES))
def test_layers_against_the_float64_helper(name):
    cfg = LAYER_CASES[name]
    m, x, g = _build(cfg, 91)
    psi = ds.layer_psi(m, dense=m.n_out * m.n_in <= 1 << 20)             # the larger cloud: a sparse float64 Psi
    want = ds.sparse_disco_with_grads(x, m.weight, m.bias, psi, m.quadrature_weights, g, m.groups)
    assert _path(m, x) == cfg["route"]
    got = _run(m, x, g)
    errs = [ds.rel_l2(a.numpy(), t.numpy()) for a, t in zip(got, want)]
    print(name, " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) <= 1e-5, errs


@pytest.mark.parametrize("name", ["groups4_of_8", "mfma_32_32"])
def test_repeats_are_bit_identical(name):
    m, x, g = _build(LAYER_CASES[name], 92)
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


@pytest.mark.parametrize("name", ["groups4_of_8", "mfma_32_32"])
def test_layer_step_replays_from_a_captured_graph(name):
    m, x, g = _build(LAYER_CASES[name], 93)
    m = m.to(DEV)
    gen = torch.Generator().manual_seed(94)
    fresh = [torch.randn(x.shape, generator=gen).to(DEV) for _ in range(2)]
    _graph_equals_eager(m, m, x.to(DEV), g.to(DEV), fresh)
