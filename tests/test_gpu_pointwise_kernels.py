"""GPU tier: the pointwise kernels of an FNO block (sc_kernels_pmlp.h: k_pmlp_fwd, k_pblock_fwd, k_pmlp_bwd and its LIN form,
k_plin_fwd / k_plin_bwd, the two reduction stages; sc_kernels_plinx.h: k_plinx_fwd / k_plinx_bwd / k_plinx_reduce) at their
tile, grid and reduction edges on an MI355X, driven through the C-ABI with free-standing descriptors
(pointwise_reference.run_case) against float64 on the host over the full tensors.

  A  tile placement, T = 1, 3, 5, 15, 61, 65 tiles of 32 pixels: one working wave, every wave in another sample, a
     workgroup straddling a sample boundary, a last workgroup of one wave, 17 partials over 16 reduction groups -- for every
     instantiation a dispatcher of sc_engine.cpp can launch.  Every output, gradient and the workspace sits between guard
     bands of one sample (a tile index one past the end lands at sample B, inside the band).
  B  the persistent tile loop: T = R - 1, R, R + 1 and 2 R + 1 with R = 4 x the kernel's workgroup cap, one gated and
     activated variant per shape id; for each backward kernel gout (skip, addend) zero outside one tile -- the tile of the
     second round, tile 0, the last tile of the first round
  C  the two reduction stages: n_wg = 1, 2, 15, 16, 17, 31, 33, cap - 1, cap partials
Every capped case asserts the workgroup count the library chose.  Every compared tensor meets the rel-L2 bar of the
existing device tests of its pass and, per element, |got - want| <= bound with the bounds of pointwise_reference (derived
from the kernels' arithmetic, no margin).  Repeats and a captured graph give identical bits; the activation is checked on
its tails against its stated error.  Out of scope: spatial >= 2^27 (the 32-bit lane byte offset; one tensor is 17 GB at 32
channels), tensors above 2^31 elements, bf16 I/O, the spectral half of FusedBlockFn."""
import pytest
import torch

import pointwise_reference as pr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _lib():
    from neuraloperator_amd import _lib
    return _lib.get_lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _cus():
    return pr.cu_count(DEV)


# ---- A ------------------------------------------------------------------------------------------------------------------------
A_CASES = [(kind, name) for kind, table in pr.TABLES.items() for name in sorted(table)]


@pytest.mark.parametrize("kind,name", A_CASES, ids=[f"{k}-{n}" for k, n in A_CASES])
def test_tile_placement_inside_guard_bands(kind, name):
    cfg = pr.TABLES[kind][name]
    cap = {"mlp_fwd": pr.PMLP_FWD_CAP, "block_fwd": pr.PBLOCK_FWD_CAP, "mlp_bwd": pr.PMLP_BWD_CAP, "block_bwd": pr.PMLP_BWD_CAP,
           "lin_bwd": pr.PLIN_BWD_CAP}.get(kind)
    expect = None if cap is None else pr.n_wg_for(cfg["T"], cap)       # (the other grids follow the CU count: run_case)
    pr.run_case(kind, _lib(), cfg, DEV, _stream(), guard=True, seed=11, expect_n_wg=expect)


def test_the_case_table_names_the_edges():
    """every instantiation a dispatcher of the pointwise section can launch appears in Table A, every tile count with
    at least one case of every kernel, and the tile counts are built as described"""
    seen = {pr.instantiation(kind, pr.TABLES[kind][name]) for kind, name in A_CASES}
    assert seen == pr.dispatcher_arms(), (pr.dispatcher_arms() - seen, seen - pr.dispatcher_arms())
    for kind, table in pr.TABLES.items():
        assert {c["T"] for c in table.values()} == set(pr.A_TILES), kind
        for c in table.values():
            assert c["B"] * c["S"] == 32 * c["T"]
    assert [pr.shape_of_tiles(t) for t in pr.A_TILES] == [(1, 32), (3, 32), (5, 32), (5, 96), (1, 32 * 61), (5, 32 * 13)]
    assert pr.n_wg_for(61, 256) == 16 and pr.n_wg_for(65, 256) == 17 and 61 % 4 == 1
    assert pr.n_wg_from_workspace((17 + 16) * pr.pmlp_np(64, 32, 64) * 4 + 256, pr.pmlp_np(64, 32, 64)) == 17


def test_the_library_counts_the_compute_units_the_grids_are_built_from():
    """k_plin_fwd and k_plinx_* size their grids by sc_cu_count(): read it back through the LEAN grid of the 32 -> 32 map
    (two workgroups per unit) and hold it to the device's multiprocessor count"""
    nbytes = _lib().pointwise_linear_workspace_bytes_ex(1, 32, 32, 32 * 4 * 4096)
    assert pr.n_wg_from_workspace(nbytes, pr.plinx_np(32, 32)) == 2 * _cus()


# ---- B ------------------------------------------------------------------------------------------------------------------------
def _b_kinds():
    """(kind, shape tag, cfg without its extents) for one gated + activated variant per shape id"""
    out = []
    for sid, ch in pr.MLP_SHAPES.items():
        out.append(("mlp_fwd", str(sid), dict(chans=ch, gate=1, act=1, bias=1, sid=sid)))
    for sid in (111, 212, 222):
        ci, ch, _ = pr.MLP_SHAPES[sid]
        out.append(("block_fwd", str(sid), dict(chans=(ci, ch), act=pr.ACT_DGRAD, bias=1, sid=sid)))
        out.append(("mlp_bwd", str(sid), dict(chans=pr.MLP_SHAPES[sid], gate=1, act=1, xpre="grad", gbias=1, sid=sid)))
    for sid in (111, 212):
        ci, ch, _ = pr.MLP_SHAPES[sid]
        out.append(("block_bwd", str(sid), dict(chans=(ci, ch), act=pr.ACT_DGRAD, sid=sid)))
    for c in (32, 64, 128):
        out.append(("lin_fwd", str(c), dict(c=c, bias=1)))
    for c in (32, 64):
        out.append(("lin_bwd", str(c), dict(c=c, addend=1, gbias=1)))
    for ci in pr.PLX_CHANS:
        for co in pr.PLX_CHANS:
            out.append(("plinx_fwd", f"{ci}_{co}", dict(ci=ci, co=co, flags=pr.XACT | pr.ACT, gated=True, pre_out=1)))
            out.append(("plinx_bwd", f"{ci}_{co}", dict(ci=ci, co=co, flags=pr.XACT | pr.XGRAD | pr.PRO, gated=True, addend=True, want_gx=1)))
            out.append(("plinx_bwd", f"{ci}_{co}_lean", dict(ci=ci, co=co, flags=0, gated=False, addend=False, want_gx=0)))
    return out


def _b_cases():
    """T = R - 1, R, R + 1 for every shape id, one 2 R + 1 per kernel at its smallest shape (R follows the cap, and the
    cap of some kernels the chip: the tile count is worked out in the test, the id names its place)"""
    cases, seen = [], set()
    for kind, tag, cfg in _b_kinds():
        which = ["R-1", "R", "R+1"]
        if (kind, tag.endswith("lean")) not in seen:
            seen.add((kind, tag.endswith("lean")))
            which.append("2R+1")
        cases += [(f"{kind}-{tag}-{w}", kind, cfg, w) for w in which]
    return cases


B_CASES = _b_cases()


def _at(kind, cfg, which):
    cap = pr.cap_of(kind, cfg, _cus())
    return pr.with_tiles(cfg, pr.round_tiles(which, cap)), cap


@pytest.mark.parametrize("tag,kind,cfg,which", B_CASES, ids=[c[0] for c in B_CASES])
def test_the_persistent_loop_and_its_ragged_last_round(tag, kind, cfg, which):
    cfg, cap = _at(kind, cfg, which)
    pr.run_case(kind, _lib(), cfg, DEV, _stream(), seed=13, expect_n_wg=cap)


M_KINDS = [("mlp_bwd-212", "mlp_bwd", dict(chans=(64, 32, 64), gate=1, act=1, xpre="pre", gbias=1, sid=212)),
           ("mlp_bwd-111-plain", "mlp_bwd", dict(chans=(32, 32, 32), gate=1, act=0, xpre=None, gbias=1, sid=111)),
           ("block_bwd-212", "block_bwd", dict(chans=(64, 32), act=pr.ACT_DGRAD, sid=212)),
           ("lin_bwd-64", "lin_bwd", dict(c=64, addend=1, gbias=1)),
           ("plinx_bwd-64_128", "plinx_bwd", dict(ci=64, co=128, flags=pr.PRO | pr.XGRAD, gated=True, addend=True, want_gx=1)),
           ("plinx_bwd-128_128", "plinx_bwd", dict(ci=128, co=128, flags=pr.PRO, gated=True, addend=True, want_gx=1)),
           ("plinx_bwd-64_64_lean", "plinx_bwd", dict(ci=64, co=64, flags=0, gated=False, addend=False, want_gx=0))]
M_CASES = [(f"{tag}-{where}", kind, cfg, where) for tag, kind, cfg in M_KINDS for where in ("second_round", "first", "last_of_round_one")]


@pytest.mark.parametrize("tag,kind,cfg,where", M_CASES, ids=[c[0] for c in M_CASES])
def test_one_marked_tile_is_the_whole_gradient(tag, kind, cfg, where):
    """T = R + 1; gout (skip, addend) is zero outside one tile: the parameter gradients are that tile's alone (bounds from
    its magnitudes: a dropped or doubled tile is an error of the size of the result), gx and gskip are exactly zero elsewhere"""
    cfg, cap = _at(kind, cfg, "R+1")
    tile = {"second_round": 4 * cap, "first": 0, "last_of_round_one": 4 * cap - 1}[where]
    got, _, _ = pr.run_case(kind, _lib(), cfg, DEV, _stream(), seed=17, mark=tile, expect_n_wg=cap)
    pr.assert_zero_outside_tile(got, cfg, tile)


# ---- C ------------------------------------------------------------------------------------------------------------------------
C_KINDS = [("mlp_bwd-212", "mlp_bwd", dict(chans=(64, 32, 64), gate=1, act=1, xpre=None, gbias=1, sid=212)),
           ("lin_bwd-64", "lin_bwd", dict(c=64, addend=0, gbias=1)),
           ("plinx_bwd-64_128", "plinx_bwd", dict(ci=64, co=128, flags=pr.PRO, gated=True, addend=False, want_gx=1)),
           ("plinx_bwd-128_128", "plinx_bwd", dict(ci=128, co=128, flags=pr.PRO, gated=True, addend=False, want_gx=1))]
C_CASES = [(f"{tag}-nwg{n}", kind, cfg, n) for tag, kind, cfg in C_KINDS for n in (1, 2, 15, 16, 17, 31, 33, "cap-1", "cap")]
# null gb1 / gb2 / ggate beside 17 partials: the dummies stay NaN
C_CASES += [("mlp_bwd-212-nwg17-no-bias-gate-grads", "mlp_bwd", dict(chans=(64, 32, 64), gate=0, act=1, xpre=None, gbias=0, sid=212), 17),
            ("lin_bwd-64-nwg17-no-gb", "lin_bwd", dict(c=64, addend=0, gbias=0), 17)]


@pytest.mark.parametrize("tag,kind,cfg,n_wg", C_CASES, ids=[c[0] for c in C_CASES])
def test_reduction_stages(tag, kind, cfg, n_wg):
    """T = 4 n_wg - 3.  k_pmlp_reduce1 (ceil(n_wg / 16) partials per group, a ragged last stride) and the final stage of
    each family; at 128 -> 128 two launches own rows 0..63 and 64..127 of gw / gb / ggate in turn through one partial
    buffer.  Guarded: a final stage writing past its rows, or a first stage past its 16 groups, meets a sentinel."""
    cap = pr.cap_of(kind, cfg, _cus())
    n = {"cap-1": cap - 1, "cap": cap}.get(n_wg, n_wg)
    pr.run_case(kind, _lib(), pr.with_tiles(cfg, 4 * n - 3), DEV, _stream(), guard=True, seed=19, expect_n_wg=n)


# ---- repeats ------------------------------------------------------------------------------------------------------------------
R_CASES = [c for c in B_CASES if c[3] == "R+1" and c[0].rsplit("-", 1)[0] in
           ("mlp_bwd-212", "block_bwd-212", "lin_bwd-64", "plinx_bwd-64_64", "plinx_bwd-128_128", "plinx_bwd-64_64_lean")]
_RUN = {"mlp_bwd": (pr.run_mlp_backward, pr.mlp_inputs), "block_bwd": (pr.run_block_backward, pr.block_inputs),
        "lin_bwd": (pr.run_linear_backward, pr.linear_inputs), "plinx_bwd": (pr.run_plinx_backward, pr.plinx_inputs)}


@pytest.mark.parametrize("tag,kind,cfg,which", R_CASES, ids=[c[0] for c in R_CASES])
def test_two_runs_give_the_same_bits(tag, kind, cfg, which):
    """the partial sums are added in a fixed order: no atomics on memory, no dependence on which workgroup finishes first"""
    cfg, _ = _at(kind, cfg, which)
    run, inputs = _RUN[kind]
    inp = inputs(cfg, 23, backward=True)
    a, b = (run(_lib(), cfg, inp, DEV, _stream()) for _ in range(2))
    assert set(a) == set(b) and len(a) >= 3
    for k in a:
        assert (a[k] is None and b[k] is None) or torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_a_capped_backward_replays_from_a_captured_graph():
    """sc_pointwise_mlp_backward_ex at 1025 tiles (k_pmlp_bwd + the two reduction stages on one stream) from a captured
    graph: the replay equals the eager call bit for bit"""
    lib = _lib()
    t = pr.second_round_tiles(pr.PMLP_BWD_CAP)
    B, S = pr.shape_of_tiles(t)
    ci, ch, co = 64, 32, 64
    cfg = dict(chans=(ci, ch, co), B=B, S=S, gate=1, act=1, xpre=None)
    assert pr.mlp_backward_n_wg(lib, cfg) == pr.PMLP_BWD_CAP
    inp = {k: v.to(DEV) for k, v in pr.mlp_inputs(cfg, 29, backward=True).items()}
    outs = [torch.empty(s, device=DEV) for s in ((B, ci, S), (ch, ci), (ch,), (co, ch), (co,), (B, co, S), (co,))]
    ws = torch.empty(lib.pointwise_mlp_workspace_bytes(B, ci, ch, co, S, 1), dtype=torch.uint8, device=DEV)
    p = lambda k: inp[k].data_ptr()

    def step():
        lib.pointwise_mlp_backward(B, ci, ch, co, S, 1, p("x"), p("w1"), p("b1"), p("w2"), p("b2"), p("skip"), p("gate"), p("gout"),
                                   *[o.data_ptr() for o in outs], ws.data_ptr(), torch.cuda.current_stream().cuda_stream)

    step()
    torch.cuda.synchronize()
    eager = [o.clone() for o in outs]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                               # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(2):
        for o in outs:
            o.fill_(float("nan"))
        ws.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for o, e in zip(outs, eager):
            assert torch.equal(o.view(torch.int32), e.view(torch.int32))


# ---- the activation on its tails -------------------------------------------------------------------------------------------
def test_the_activation_on_its_tails_on_every_route():
    got = pr.run_activation_routes(_lib(), DEV, _stream())
    pr.check_activation(got)
    names = list(got["gelu"])
    for n in names[1:]:                                      # the pair and the scalar forms: the same bits
        assert torch.equal(got["gelu"][n].view(torch.int32), got["gelu"][names[0]].view(torch.int32)), (names[0], n)


# ---- the Python routes ------------------------------------------------------------------------------------------------------
def _f64_mlp(x, w1, b1, w2, b2, skip, gate):
    import torch.nn.functional as F
    h = F.gelu(torch.einsum("hc,bcxy->bhxy", w1, x) + b1[None, :, None, None])
    return F.gelu(torch.einsum("oh,bhxy->boxy", w2, h) + b2[None, :, None, None] + gate[None, :, None, None] * skip)


@pytest.mark.parametrize("grid,engine", [((32, 33), True), ((33, 31), False)], ids=["32x33-engine", "33x31-torch"])
def test_python_routes_take_the_engine_at_33_tiles_and_torch_at_1023_points(grid, engine):
    """blocks.fused_linear / fused_channel_mlp on 1056 points (33 tiles: the engine's node) and on 1023 (no multiple of
    32: the torch composition), both against float64 autograd at the bar of the existing tests"""
    from neuraloperator_amd import blocks as nb
    g = torch.Generator().manual_seed(31)
    mk = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc)
    B, c, ch = 2, 64, 32
    host = [mk(B, c, *grid), mk(ch, c, sc=c ** -0.5), mk(ch), mk(c, ch, sc=ch ** -0.5), mk(c), mk(B, c, *grid), mk(c)]
    cot = mk(B, c, *grid)
    dl = [t.to(DEV).requires_grad_(True) for t in host]
    out = nb.fused_channel_mlp(dl[0], dl[1], dl[2], dl[3], dl[4], skip_src=dl[5], gate=dl[6], activation="gelu")
    assert ("PointwiseMLP" in type(out.grad_fn).__name__) == engine, type(out.grad_fn).__name__
    out.backward(cot.to(DEV))
    rl = [t.double().requires_grad_(True) for t in host]
    ref = _f64_mlp(*rl)
    ref.backward(cot.double())
    assert pr.rel_l2(out.detach().cpu().numpy(), ref.detach().numpy()) < 3e-6
    for a, b in zip(dl, rl):
        assert pr.rel_l2(a.grad.cpu().numpy(), b.grad.numpy()) < 1e-5
    # the 1 x 1 map
    xl, wl, bl = (t.to(DEV).requires_grad_(True) for t in (host[0], mk(c, c, sc=c ** -0.5), host[4]))
    o2 = nb.fused_linear(xl, wl, bl)
    assert ("PointwiseLinear" in type(o2.grad_fn).__name__) == engine, type(o2.grad_fn).__name__
    o2.backward(cot.to(DEV))
    xr, wr, br = (t.detach().cpu().double().requires_grad_(True) for t in (xl, wl, bl))
    r2 = torch.einsum("oc,bcxy->boxy", wr, xr) + br[None, :, None, None]
    r2.backward(cot.double())
    assert pr.rel_l2(o2.detach().cpu().numpy(), r2.detach().numpy()) < 3e-6
    for a, b in zip((xl, wl, bl), (xr, wr, br)):
        assert pr.rel_l2(a.grad.cpu().numpy(), b.grad.numpy()) < 1e-5


def test_python_block_route_on_33_tiles_and_on_1023_points():
    """blocks.fused_block_forward on a 32 x 33 grid (FusedBlockFn) and on 33 x 31 (the op sequence) against the block
    itself, at the bar of test_fused_block_forward_matches_op_sequence"""
    from block_standin import Blocks
    from neuraloperator_amd import blocks as nb
    from test_gpu_parity import TOL, _block_oracle
    torch.manual_seed(6)
    blk = Blocks(64, (8, 8)).to(DEV)
    with torch.no_grad():
        for q in blk.parameters():
            if q.is_complex():
                q.mul_(4.0)
        blk.channel_mlp_skips[0].weight.copy_(torch.randn_like(blk.channel_mlp_skips[0].weight))
    for grid, engine in (((32, 33), True), ((33, 31), False)):
        x, g = torch.randn(2, 64, *grid, device=DEV), torch.randn(2, 64, *grid, device=DEV)
        nodes, orig = [], nb.FusedBlockFn.apply
        nb.FusedBlockFn.apply = staticmethod(lambda *a: (nodes.append(1), orig(*a))[1])
        try:
            blk.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(True)
            y = nb.fused_block_forward(blk, xi, 0)
            y.backward(g)
        finally:
            nb.FusedBlockFn.apply = orig
        assert nodes == ([1] if engine else []), (grid, nodes)
        gp1 = {n: q.grad.clone() for n, q in blk.named_parameters() if q.grad is not None}
        yo, gxo, gpo = _block_oracle(blk, x, g, 0)
        assert pr.rel_l2(y.detach().cpu().numpy(), yo.numpy()) < TOL and pr.rel_l2(xi.grad.cpu().numpy(), gxo.numpy()) < TOL
        assert set(gpo) == set(gp1)
        for n in gpo:
            a, b = gp1[n].cpu(), gpo[n]
            a, b = (torch.view_as_real(a), torch.view_as_real(b)) if a.is_complex() else (a, b)
            assert pr.rel_l2(a.numpy(), b.numpy()) < 2e-5, n
