"""GPU tier: the graph neural operator layer on an MI355X -- every recorded fixture forward and backward at the bars of
tests/test_gno_reference.py, a larger search + integral against the float64 helper, a low-channel high-degree case,
bit-identical repeats, and one IntegralTransform step replayed from a captured graph."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gno_reference as gr
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("name", sorted(gr.CASES))
def test_gno_block_matches_the_recorded_reference(name):
    rec = load_golden("gno_" + name)
    errs = gr.check_case_against_record(gr.run_engine_case(gr.CASES[name], rec, DEV), rec)
    print(name, {k: f"{v:.1e}" for k, v in errs.items()})


def _integral_case(n, m, d, r, c, batch, seed, hidden=16):
    """search + linear transform (mean) on the engine and in the float64 helper; queries inside the 1e-5 r band are
    removed before both sides run.  Returns (removed share, engine module, inputs, helper output and gradients)."""
    from neuraloperator_amd import IntegralTransform, NeighborSearch
    g = torch.Generator().manual_seed(seed)
    y, x = torch.rand(n, d, generator=g), torch.rand(m, d, generator=g)
    band = gr.band_queries(y.numpy(), x.numpy(), r)
    x = x[torch.from_numpy(~band)]
    f = torch.randn(batch, n, c, generator=g)
    it = IntegralTransform(channel_mlp_layers=[2 * d, hidden, c], reduction="mean").to(DEV)
    nbrs = NeighborSearch()(y.to(DEV), x.to(DEV), r)
    ref = gr.radius_search(y.numpy(), x.numpy(), r)
    np.testing.assert_array_equal(nbrs["neighbors_row_splits"].cpu().numpy(), ref["neighbors_row_splits"])
    np.testing.assert_array_equal(nbrs["neighbors_index"].cpu().numpy(), ref["neighbors_index"])
    fd = f.to(DEV).requires_grad_(True)
    gout = torch.randn(batch, x.shape[0], c, generator=g)

    def step():
        fd.grad = None
        it.zero_grad(set_to_none=True)
        out = it(y.to(DEV), nbrs, x=x.to(DEV), f_y=fd)
        out.backward(gout.to(DEV))
        return [out.detach().clone(), fd.grad.clone()] + [p.grad.clone() for p in it.parameters()]

    sd = it.state_dict()
    Ws = [v.detach().cpu().double().requires_grad_(True) for k, v in sd.items() if k.endswith("weight")]
    bs = [v.detach().cpu().double().requires_grad_(True) for k, v in sd.items() if k.endswith("bias")]
    f64 = f.double().requires_grad_(True)
    h = gr.integral_transform(y.double(), x.double(), {k: torch.from_numpy(v) for k, v in ref.items()}, Ws, bs, f_y=f64,
                              reduction="mean")
    h.backward(gout.double())
    refs = [h.detach(), f64.grad] + [t.grad for pair in zip(Ws, bs) for t in pair]
    return band.mean(), step, refs, int(ref["neighbors_row_splits"][-1]) / max(x.shape[0], 1)


def test_larger_case_against_the_helper_and_bitwise_repeat():
    removed, step, refs, _ = _integral_case(5000, 3000, 3, 0.1, 32, 2, seed=11)
    print(f"queries removed: {100 * removed:.2f} %")
    assert removed <= 0.01
    a, b = step(), step()
    for i, (t, r) in enumerate(zip(a, refs)):
        err = gr.rel_l2(t.cpu().numpy(), r.numpy())
        print(i, f"{err:.1e}")
        assert err <= (1e-5 if i < 2 else 2e-5), (i, err)
    assert all(torch.equal(u, v) for u, v in zip(a, b))      # forward and backward launched twice: the same bits


def test_three_channels_and_average_degree_above_64():
    removed, step, refs, degree = _integral_case(600, 200, 2, 0.25, 3, 2, seed=12, hidden=8)
    assert degree > 64 and removed <= 0.01
    for i, (t, r) in enumerate(zip(step(), refs)):
        err = gr.rel_l2(t.cpu().numpy(), r.numpy())
        assert err <= (1e-5 if i < 2 else 2e-5), (i, err)


def test_integral_transform_step_replays_from_a_captured_graph():
    """the search synchronises (it sizes its outputs) and stays outside; the transform with precomputed neighbours,
    forward and backward, is captured and replayed on new inputs"""
    from neuraloperator_amd import IntegralTransform, NeighborSearch
    g = torch.Generator().manual_seed(5)
    y, x = torch.rand(300, 3, generator=g).to(DEV), torch.rand(200, 3, generator=g).to(DEV)
    nbrs = NeighborSearch()(y, x, 0.3)
    it = IntegralTransform(channel_mlp_layers=[6, 16, 4]).to(DEV)
    f = torch.randn(2, 300, 4, generator=g).to(DEV).requires_grad_(True)
    gout = torch.randn(2, 200, 4, generator=g).to(DEV)

    def eager(fv):
        fv = fv.detach().clone().requires_grad_(True)
        out = it(y, nbrs, x=x, f_y=fv)
        out.backward(gout)
        return out.detach().clone(), fv.grad.clone()

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                               # warm-up off the capture, as torch asks -- on a leaf of
        warm = f.detach().clone().requires_grad_(True)       # its own: the captured leaf's gradient accumulator must be
        for _ in range(2):                                   # created on the capture stream, not on this one
            it(y, nbrs, x=x, f_y=warm).backward(gout)
    torch.cuda.current_stream().wait_stream(s)
    it.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = it(y, nbrs, x=x, f_y=f)
        out.backward(gout)
    for seed in (6, 7):
        new = torch.randn(2, 300, 4, generator=torch.Generator().manual_seed(seed)).to(DEV)
        with torch.no_grad():
            f.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        want_out, want_g = eager(new)
        assert torch.equal(out, want_out) and torch.equal(f.grad, want_g)
