"""GPU tier: the chunked kernel MLP of the GNO layer (sc_kernels_gno_mlp.h) on an MI355X against the float64 helper
(tests/gno_mlp_reference.py): every case of the table through engine.EdgeMlpFn, the C-ABI on free-standing descriptors,
chunk sizes against each other, a captured step, and the peak memory of both routes against the edge count."""
import numpy as np
import pytest
import torch

import gno_mlp_reference as mr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from neuraloperator_amd import _lib
    return _lib.get_lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("name", sorted(mr.CASES))
def test_edge_mlp_fn_against_float64(name):
    from neuraloperator_amd import engine
    before = engine.EdgeMlpFn.calls
    got = mr.run_fn(name, DEV)
    assert engine.EdgeMlpFn.calls == before + 1
    mr.check(name, got)
    if name == "bad_index":                                  # an edge without a neighbour: the chain of a zero row
        t = mr.build(name)
        zero_row = mr.chain(t, t["Py"], t["Px"], t["b0"], t["Ws"], t["bs"])[list(t["cfg"]["bad"])]
        torch.testing.assert_close(got["K"][list(t["cfg"]["bad"])].cpu(), zero_row, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", ["e389_odd_widths", "batched", "bad_index", "e0"])
def test_cabi_on_a_free_standing_descriptor(lib, name):
    with torch.cuda.device(DEV):
        got = mr.run_cabi(lib, name, DEV, stream=_stream())
    mr.check(name, got)
    assert mr.same_bits(got, mr.run_fn(name, DEV))


def test_weight_gradients_across_chunks(lib):
    name = "rows_against_chunks"
    with torch.cuda.device(DEV):
        small, again = (mr.run_cabi(lib, name, DEV, chunk=mr.TILE, stream=_stream()) for _ in range(2))
        whole, whole_again = (mr.run_cabi(lib, name, DEV, chunk=0, stream=_stream()) for _ in range(2))
    mr.check(name, small)
    mr.check(name, whole)
    assert mr.same_bits(small, again) and mr.same_bits(whole, whole_again)
    assert torch.equal(small["K"], whole["K"])               # a row of K does not depend on the chunk it falls into


def test_refusals(lib):
    from neuraloperator_amd import _lib
    t = mr.build("e20")
    dev = {k: t[k].to(DEV) for k in ("Py", "Px", "b0", "gK")}
    Ws, bs = [w.to(DEV) for w in t["Ws"]], [b.to(DEV) for b in t["bs"]]
    args = (dev["Py"].data_ptr(), dev["Px"].data_ptr(), dev["b0"].data_ptr(), [w.data_ptr() for w in Ws],
            [b.data_ptr() for b in bs])
    buf = torch.zeros(1 << 16, device=DEV)
    for over in (dict(widths=[16, 513, 3]), dict(widths=[16], n_layers=1), dict(widths=[8] * 8, n_layers=9),
                 dict(chunk=100)):
        d, keep = mr.desc_of(t, DEV, over.pop("chunk", mr.TILE), **over)
        assert lib.edge_mlp_workspace_bytes(d) == 0
        with pytest.raises(_lib.EngineError):
            lib.edge_mlp_forward(d, *args, buf.data_ptr(), buf.data_ptr(), buf.numel() * 4, _stream())
    d, keep = mr.desc_of(t, DEV, mr.TILE)
    nbytes = lib.edge_mlp_workspace_bytes(d)
    ws = torch.zeros(nbytes // 4, device=DEV)
    with pytest.raises(_lib.EngineError, match="workspace"):
        lib.edge_mlp_forward(d, *args, buf.data_ptr(), ws.data_ptr(), nbytes - 4, _stream())
    g = [torch.zeros_like(x) for x in (dev["Py"], dev["Px"], *Ws, *bs)]
    with pytest.raises(_lib.EngineError, match="workspace"):
        lib.edge_mlp_backward(d, *args, dev["gK"].data_ptr(), g[0].data_ptr(), g[1].data_ptr(),
                              [x.data_ptr() for x in g[2:4]], [x.data_ptr() for x in g[4:6]], ws.data_ptr(), nbytes - 4,
                              _stream())
    torch.cuda.synchronize()


def _transform(hidden, c_in, c_out, route="auto"):
    from neuraloperator_amd import IntegralTransform
    torch.manual_seed(11)
    return IntegralTransform(channel_mlp_layers=[c_in, *hidden, c_out], kernel_route=route).to(DEV)


def test_fused_on_a_relu_network_raises():
    import torch.nn.functional as F
    from neuraloperator_amd import IntegralTransform
    from neuraloperator_amd.gno import kernel_route
    t = mr.build("e20")
    nbrs = {"neighbors_index": t["index"].to(DEV), "neighbors_row_splits": t["splits"].to(DEV)}
    y, x = torch.rand(t["cols"], 2, device=DEV), torch.rand(t["rows"], 2, device=DEV)
    f = torch.randn(t["cols"], 3, device=DEV)
    it = IntegralTransform(channel_mlp_layers=[4, 8, 3], channel_mlp_non_linearity=F.relu).to(DEV)
    it(y, nbrs, x, f)
    with pytest.raises(ValueError, match="fused"):
        with kernel_route("fused"):
            it(y, nbrs, x, f)


def test_fused_step_replays_from_a_captured_graph():
    """the transform on the fused route with precomputed neighbours, forward and backward, captured and replayed on new
    inputs: every launch of every chunk is stream ordered and nothing waits for the device"""
    from neuraloperator_amd import NeighborSearch, engine
    g = torch.Generator().manual_seed(5)
    y, x = torch.rand(300, 3, generator=g).to(DEV), torch.rand(200, 3, generator=g).to(DEV)
    nbrs = NeighborSearch()(y, x, 0.3)
    it = _transform((33, 16), 6, 4, route="fused")
    f = torch.randn(2, 300, 4, generator=g).to(DEV).requires_grad_(True)
    gout = torch.randn(2, 200, 4, generator=g).to(DEV)

    import copy
    twin = copy.deepcopy(it)                                 # the same parameters, gradients of its own

    def eager(fv):
        fv = fv.detach().clone().requires_grad_(True)
        twin.zero_grad(set_to_none=True)
        out = twin(y, nbrs, x=x, f_y=fv)
        out.backward(gout)
        return out.detach(), fv.grad, [p.grad for p in twin.parameters()]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                               # warm-up off the capture, on a leaf of its own
        warm = f.detach().clone().requires_grad_(True)
        for _ in range(2):
            it(y, nbrs, x=x, f_y=warm).backward(gout)
    torch.cuda.current_stream().wait_stream(s)
    it.zero_grad(set_to_none=True)
    before = engine.EdgeMlpFn.calls
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = it(y, nbrs, x=x, f_y=f)
        out.backward(gout)
    assert engine.EdgeMlpFn.calls == before + 1
    for seed in (6, 7):
        new = torch.randn(2, 300, 4, generator=torch.Generator().manual_seed(seed)).to(DEV)
        with torch.no_grad():
            f.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        want_out, want_g, want_p = eager(new)
        assert torch.equal(out, want_out) and torch.equal(f.grad, want_g)
        for (k, p), w in zip(it.named_parameters(), want_p):
            if k.startswith("channel_mlp.fcs.0."):           # torch's own products of gPy / gPx with the points: the
                assert mr.rel_l2(p.grad.cpu(), w.cpu()) <= 2e-5, k    # library may pick another kernel under capture
            else:                                            # what sc_edge_mlp_backward wrote
                assert torch.equal(p.grad, w), k


def _peak_of_a_step(n_edges, route):
    """max_memory_allocated of one forward + backward of IntegralTransform (256, 128) -> 8 on a graph of n_edges edges,
    b = 1; the graph's own arrays are allocated when the count starts and so are part of it"""
    from neuraloperator_amd.gno import kernel_route
    rows, cols, c_out = 2000, 2000, 8                        # the points stay: only edge-sized tensors grow
    rng = np.random.default_rng(n_edges)
    splits, index = mr.gr.random_csr(rng, rows, cols, np.full(rows, n_edges // rows, np.int64))
    it = _transform((256, 128), 4, c_out)
    g = torch.Generator().manual_seed(1)
    y, x = torch.rand(cols, 2, generator=g).to(DEV), torch.rand(rows, 2, generator=g).to(DEV)
    f = torch.randn(cols, c_out, generator=g).to(DEV).requires_grad_(True)
    gout = torch.randn(rows, c_out, generator=g).to(DEV)
    nbrs = {"neighbors_index": torch.from_numpy(index).to(DEV), "neighbors_row_splits": torch.from_numpy(splits).to(DEV)}
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    with kernel_route(route):
        out = it(y, nbrs, x=x, f_y=f)
        out.backward(gout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(DEV)
    return peak, len(index)


def test_peak_memory_does_not_grow_with_edges_times_hidden_width():
    """growth of the peak between E1 ~ 60 k and E2 ~ 120 k edges against (E2 - E1) (8 b c_out + 32) + 1 MiB: K saved, gK,
    the int64 index and the two int32 transpose arrays.  The fused route stays within it; the edge route, whose autograd
    nodes keep E x 256 and E x 128 tensors, does not."""
    c_out, b = 8, 1
    growth = {}
    for route in ("fused", "edges"):
        _peak_of_a_step(60000, route)                        # the libraries' own first-use workspaces are allocated here
        p1, e1 = _peak_of_a_step(60000, route)
        p2, e2 = _peak_of_a_step(120000, route)
        growth[route] = (p2 - p1, (e2 - e1) * (8 * b * c_out + 32) + (1 << 20))
    print({k: (f"{v[0] / 2 ** 20:.1f} MiB", f"bound {v[1] / 2 ** 20:.1f} MiB") for k, v in growth.items()})
    assert growth["fused"][0] <= growth["fused"][1], growth
    assert growth["edges"][0] > growth["edges"][1], growth
