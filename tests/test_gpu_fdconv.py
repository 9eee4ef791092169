"""GPU tier: FiniteDifferenceConvolution on an MI355X -- every recorded fixture at the bars of
tests/test_fdconv_reference.py, the issue-sized and the remaining matrix-core channel pairs plus a 3-d general-route
case against the float64 helper on the host, the route each takes, bit-identical repeats of both routes, and one
forward + backward step replayed from a captured graph."""
import pytest
import torch

import fdconv_reference as fr
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _path(cfg, h):
    from neuraloperator_amd import _lib
    d = _lib.ScEngineLib.fdconv_desc(dims=cfg["dims"], batch=cfg["batch"], c_in=cfg["c_in"], c_out=cfg["c_out"],
                                     k=cfg["k"], groups=cfg["groups"], padding=cfg["padding"], inv_h=1.0 / h)
    return _lib.get_lib().fdconv_path(d)


@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_layer_matches_the_recorded_reference(name):
    cfg, rec = fr.CASES[name], load_golden("fdconv_" + name)
    x, w, g, h = (torch.from_numpy(rec["x"]), torch.from_numpy(rec["weight"]), torch.from_numpy(rec["g"]),
                  float(rec["grid_width"]))
    assert _path(cfg, h) == cfg["route"]
    out, gx, gw, _ = fr.run_module(cfg, x, w, g, h, DEV)
    bars = fr.record_bars(cfg, rec)
    got, want = (out, gx, gw), (rec["out"], rec["grad:x"], rec["grad:weight"])
    raw = tuple(fr.rel_l2(a, b) for a, b in zip(got, want))
    print(name, "errors", " ".join(f"{e:.2e}" for e in raw), "bars", " ".join(f"{b:.2e}" for b in bars))
    if cfg["smooth"]:
        print(name, "ratio to the verbatim fp32 class's own error",
              " ".join(f"{2 * e / b:.2f}" for e, b in zip(raw, bars)))
    fr.check_against(cfg, got, want, bars, fr.magnitudes(x, w, g, h, cfg["groups"], cfg["padding"]))


# no fixtures (too large to commit): the float64 helper on the host is the reference
HELPER_CASES = {
    **fr.LIVE_CASES,
    "2d_mfma_zeros_64_128": fr._case((16, 16), 64, 128, padding="zeros", batch=1, route=fr.MFMA),
    "2d_mfma_periodic_128_32": fr._case((4, 36), 128, 32, route=fr.MFMA),
    "2d_mfma_periodic_64_64": fr._case((40, 72), 64, 64, route=fr.MFMA),
    "3d_k3_zeros_33_31": fr._case((6, 9, 70), 33, 31, padding="zeros"),
}


@pytest.mark.parametrize("name", sorted(HELPER_CASES))
def test_larger_cases_against_the_float64_helper(name):
    cfg = HELPER_CASES[name]
    x, w, g = fr.case_inputs(cfg, 91)
    h = fr.grid_width_of(cfg)
    assert _path(cfg, h) == cfg["route"]
    out, gx, gw, _ = fr.run_module(cfg, x, w, g, h, DEV)
    want = [t.numpy() for t in fr.fdconv_with_grads(x, w, g, h, cfg["groups"], cfg["padding"])]
    # where the stencil cancels (smooth field): twice the error of the reference's own formula in fp32 on the same input
    bars = fr.smooth_bars(x, w, g, h, cfg["groups"], cfg["padding"], want) if cfg["smooth"] else (1e-5, 1e-5, 1e-5)
    errs = fr.check_against(cfg, (out, gx, gw), want, bars)
    print(name, " ".join(f"{e:.2e}" for e in errs), "bars", " ".join(f"{b:.2e}" for b in bars))


@pytest.mark.parametrize("name", ["2d_mfma_periodic_32", "2d_k3_replicate_g2", "3d_k3_periodic", "1d_k5_reflect_depthwise"])
def test_repeats_are_bit_identical(name):
    cfg = fr.CASES[name]
    x, w, g = fr.case_inputs(cfg, 92)
    h = fr.grid_width_of(cfg)
    a, b = fr.run_module(cfg, x, w, g, h, DEV)[:3], fr.run_module(cfg, x, w, g, h, DEV)[:3]
    assert all((u == v).all() for u, v in zip(a, b))


@pytest.mark.parametrize("name", ["2d_mfma_periodic_32", "2d_k5_reflect"])
def test_step_replays_from_a_captured_graph(name):
    from neuraloperator_amd import FiniteDifferenceConvolution
    cfg = fr.CASES[name]
    x0, w, g = fr.case_inputs(cfg, 93)
    h = fr.grid_width_of(cfg)
    m = FiniteDifferenceConvolution(**fr.module_kwargs(cfg))
    with torch.no_grad():
        m.weight.copy_(w)
    m = m.to(DEV)
    gout = g.to(DEV)
    x = x0.to(DEV).requires_grad_(True)

    def eager(xv):
        xv = xv.detach().clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        out = m(xv, h)
        out.backward(gout)
        return out.detach().clone(), xv.grad.clone(), m.weight.grad.clone()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                               # warm-up off the capture, on a leaf of its own
        warm = x0.to(DEV).requires_grad_(True)
        for _ in range(2):
            m(warm, h).backward(gout)
    torch.cuda.current_stream().wait_stream(s)
    m.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(x, h)
        out.backward(gout)
    gw_static = m.weight.grad
    for seed in (94, 95):
        new = fr.case_inputs(cfg, seed)[0].to(DEV)
        with torch.no_grad():
            x.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        got = (out.detach().clone(), x.grad.clone(), gw_static.clone())
        want = eager(new)
        m.weight.grad = gw_static
        assert all(torch.equal(u, v) for u, v in zip(got, want))
