"""GPU tier: the attention kernel integral on an MI355X -- every recorded fixture at the bar of
tests/test_attention_reference.py, the descriptor list of the emulation tier through the C-ABI on the device, layers that
cross the chunk, tile and lane-layout edges on both routes against the float64 helper on the host, the route each takes,
bit-identical
repeats, and one forward + backward step of a layer replayed from a captured graph."""
import pytest
import torch

import attention_reference as ar
from neuraloperator_amd import AttentionKernelIntegral, RotaryEmbedding2D, attention

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _to_dev(t):
    out = {k: v.to(DEV) for k, v in t.items()}
    for k in ("u_src", "u_qry"):
        if k in out:
            out[k].requires_grad_(True)
    return out


def _step(m, emb, t):
    m.zero_grad(set_to_none=True)
    for k in ("u_src", "u_qry"):
        if k in t:
            t[k].grad = None
    with attention.route("engine"):                          # ValueError where the call is not the engine's
        out = ar.call_layer(m, emb, t)
    out.backward(t["g"])
    torch.cuda.synchronize()
    return out.detach().cpu(), {k: v.cpu() for k, v in ar.grads_of(m, t).items()}


@pytest.mark.parametrize("name", sorted(ar.CASES))
def test_layer_matches_the_recorded_reference(name):
    cfg, rec = ar.CASES[name], ar.load_record(name)
    m, emb = ar.build_layer(AttentionKernelIntegral, RotaryEmbedding2D, cfg, ar.SEEDS[name])
    m, emb = m.to(DEV), None if emb is None else emb.to(DEV)
    t = _to_dev({k: torch.from_numpy(rec[k]) for k in ("u_src", "pos_src", "u_qry", "pos_qry", "weights", "g") if k in rec})
    out, grads = _step(m, emb, t)
    errs = {"out": ar.rel_l2(out.numpy(), rec["out"])}
    errs.update({"grad:" + k: ar.rel_l2(g.numpy(), rec["grad:" + k]) for k, g in grads.items()})
    assert set(errs) == {k for k in rec if k == "out" or k.startswith("grad:")}
    print(name, " ".join(f"{k}={e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= ar.tolerance(rec, k), (k, e)


@pytest.mark.parametrize("name", sorted(ar.DESC_CASES))
def test_descriptors_against_the_float64_helper(name):
    from neuraloperator_amd import _lib
    cfg = ar.DESC_CASES[name]
    args = ar.desc_inputs(cfg, 41)
    got = ar.run_descriptor(_lib.get_lib(), cfg, *args, device=DEV, guard=True)[:5]    # guards compared bit for bit
    assert all(bool(torch.isfinite(t).all()) for t in got)
    errs = ar.desc_errors(got, cfg, args)
    print(name, " ".join(f"{k}={e:.1e}" for k, e in errs.items()))
    assert max(errs.values()) <= ar.BAR, errs


def _layer(c, out, heads, d, n, batch, **kw):
    return ar.case(c, out, heads, d, n, batch, **kw)


LAYER_CASES = {
    # matrix-core route (D = 32, 64, 128): one past a chunk, which is also one past a tile of the per-point kernels
    "d32_one_past_a_chunk": _layer(16, 64, 2, 32, ar.CHUNK + 1, 2, unit_pos=True),
    "d32_n1000": _layer(32, 32, 1, 32, 1000, 2),
    "d64_one_past_a_chunk": _layer(8, 64, 1, 64, ar.CHUNK + 1, 2, unit_pos=True),
    "d64_n1000_weights": _layer(24, 128, 2, 64, 1000, 1, weights=True),
    "d128_one_past_a_chunk": _layer(8, 16, 1, 128, ar.CHUNK + 1, 1, unit_pos=True),
    "d128_n1000": _layer(16, 128, 1, 128, 1000, 2, unit_pos=True),
    # vector route
    "d36_n300": _layer(10, 72, 2, 36, 300, 2, unit_pos=True),
    "d6_rot1_n300": _layer(6, 6, 1, 6, 300, 1, pos_dim=1, unit_pos=True),
    "n20000_79_partials_hd128": _layer(16, 128, 4, 32, 20000, 1, unit_pos=True),
    "cross_weights_d12_n513": _layer(9, 24, 2, 12, 2 * ar.CHUNK + 1, 2, cross=True, weights=True, unit_pos=True),
    "batch5_heads3_d12_no_rotary": _layer(7, 5, 3, 12, 130, 5, rotary=False),
}


def _build(name, seed):
    cfg = LAYER_CASES[name]
    m, emb = ar.build_layer(AttentionKernelIntegral, RotaryEmbedding2D, cfg, seed)
    return cfg, m, emb, ar.case_inputs(cfg, seed)


@pytest.mark.parametrize("name", sorted(LAYER_CASES))
def test_layers_against_the_float64_helper(name):
    from neuraloperator_amd import _lib
    cfg, m, emb, t = _build(name, 51)
    assert cfg["n"] <= 20000 and (cfg["n"] < 20000 or cfg["heads"] * cfg["d"] == 128)
    d = _lib.ScEngineLib.attn_desc(batch=cfg["batch"], n_src=cfg["n"], n_qry=cfg["n"], heads=cfg["heads"], head_dim=cfg["d"],
                                   rotary=cfg["pos_dim"] if cfg["rotary"] else 0, has_weights=int(cfg["weights"]))
    assert _lib.get_lib().attn_path(d) == ar.route_of(cfg["d"]) == (ar.MFMA if name.startswith(("d32", "d64", "d128", "n20000"))
                                                                    else ar.VECTOR)
    want_out, want = ar.layer_with_grads64(m, emb, t["u_src"], t["pos_src"], t.get("u_qry"), t.get("pos_qry"),
                                           t.get("weights"), t["g"])
    out, grads = _step(m.to(DEV), None if emb is None else emb.to(DEV), _to_dev(t))
    errs = {"out": ar.rel_l2(out.numpy(), want_out.numpy())}
    errs.update({k: ar.rel_l2(g.numpy(), want[k].numpy()) for k, g in grads.items()})
    assert set(errs) == {"out"} | set(want)
    print(name, " ".join(f"{k}={e:.2e}" for k, e in errs.items()))
    assert max(errs.values()) <= ar.BAR, errs


@pytest.mark.parametrize("name", ["d32_one_past_a_chunk", "d36_n300", "cross_weights_d12_n513"])
def test_repeats_are_bit_identical(name):
    cfg, m, emb, t = _build(name, 52)
    m, emb, t = m.to(DEV), None if emb is None else emb.to(DEV), _to_dev(t)
    (o1, g1), (o2, g2) = _step(m, emb, t), _step(m, emb, t)
    assert torch.equal(o1, o2) and all(torch.equal(g1[k], g2[k]) for k in g1)


@pytest.mark.parametrize("name", ["d32_one_past_a_chunk", "d36_n300"])
def test_layer_step_replays_from_a_captured_graph(name):
    """one forward + backward step captured on a single stream and replayed on new inputs: equal to eager bit for bit"""
    cfg, m, emb, t = _build(name, 53)
    m, emb, t = m.to(DEV), emb.to(DEV), _to_dev(t)
    params = list(m.parameters())
    pos, gout = t["pos_src"], t["g"]

    def call(xv):
        with attention.route("engine"):
            return m(xv, pos, positional_embedding_module=emb)

    def eager(xv):
        xv = xv.detach().clone().requires_grad_(True)
        m.zero_grad(set_to_none=True)
        out = call(xv)
        out.backward(gout)
        return [out.detach().clone(), xv.grad.clone()] + [p.grad.clone() for p in params]

    x = t["u_src"].detach().clone().requires_grad_(True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                               # warm-up off the capture, on a leaf of its own
        warm = x.detach().clone().requires_grad_(True)
        for _ in range(2):
            call(warm).backward(gout)
    torch.cuda.current_stream().wait_stream(s)
    m.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = call(x)
        out.backward(gout)
    static = [p.grad for p in params]
    gen = torch.Generator().manual_seed(54)
    for _ in range(2):
        new = torch.randn(x.shape, generator=gen).to(DEV)
        with torch.no_grad():
            x.copy_(new)
        graph.replay()
        torch.cuda.synchronize()
        got = [out.detach().clone(), x.grad.clone()] + [g.clone() for g in static]
        want = eager(new)
        for p, g in zip(params, static):
            p.grad = g
        assert all(torch.equal(u, v) for u, v in zip(got, want))
