"""CPU tier: the 1 x 1 maps with the block's pointwise operations in their load / store paths (csrc/sc_kernels_plinx.h, round 6)
in host emulation against the same computation in torch (float64 + autograd): every channel pair that needs its own
structure (rectangular, 128 -> 128 = two launches for the weight gradient), every option alone and all together, and the
two-pass form of the ChannelMLP + soft-gating skip + GELUs (channel_mlp.py:82-119, skip_connections.py:53-130,
fno_block.py:392-414) that blocks.PointwiseMLP2Fn / FusedBlockFn run for channel counts without a one-pass kernel."""
import pytest
import torch
import torch.nn.functional as F

import pointwise_reference as pr
from engine_runner import emu_lib, rel_l2
from neuraloperator_amd import _lib

TOL = 3e-6
XACT, ACT, PRO, XGRAD = _lib.SC_PLX_XACT, _lib.SC_PLX_ACT, _lib.SC_PLX_PRO, _lib.SC_PLX_XGRAD


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


def p(t):
    return 0 if t is None else t.data_ptr()


def _fwd_ref(x, w, b, skip, gate, flags):
    return pr.plinx64(x, w, b, skip, gate, flags)            # float64: tests/pointwise_reference.py


@pytest.mark.parametrize("ci,co", [(32, 64), (128, 64), (64, 128), (128, 128), (128, 32)])
@pytest.mark.parametrize("flags,gated,bias", [(0, False, True), (XACT | ACT, True, True), (ACT, True, False), (XACT, False, False)])
def test_forward(lib, ci, co, flags, gated, bias):
    g = torch.Generator().manual_seed(ci + 3 * co + flags)
    B, S = 2, 96
    x = torch.randn(B, ci, S, generator=g)
    w = torch.randn(co, ci, generator=g) / ci ** 0.5
    b = torch.randn(co, generator=g) if bias else None
    skip = torch.randn(B, co, S, generator=g) if gated else None
    gate = torch.randn(co, generator=g) if gated else None
    out, pre = torch.full((B, co, S), float("nan")), torch.full((B, co, S), float("nan"))
    lib.pointwise_linear_forward_ex(B, ci, co, S, flags, p(x), p(w), p(b), p(skip), p(gate), p(out), p(pre), 0)
    d = lambda t: None if t is None else t.double()
    ro, rz = _fwd_ref(d(x), d(w), d(b), d(skip), d(gate), flags)
    assert rel_l2(out.numpy(), ro.numpy()) < TOL and rel_l2(pre.numpy(), rz.numpy()) < TOL
    out2 = torch.full((B, co, S), float("nan"))
    lib.pointwise_linear_forward_ex(B, ci, co, S, flags, p(x), p(w), p(b), p(skip), p(gate), p(out2), 0, 0)      # no pre_out
    assert torch.equal(out2, out)


@pytest.mark.parametrize("ci,co", [(32, 64), (128, 64), (64, 128), (128, 128), (64, 32)])
@pytest.mark.parametrize("flags,gated,addend", [(0, False, False), (XACT | XGRAD | PRO, True, False), (XGRAD, False, True),
                                                (PRO, True, True)])
def test_backward(lib, ci, co, flags, gated, addend):
    """out = act(W xin + gate (.) skip), loss = <out, gout> (+ <x-branch, addend>): every gradient of the pass against autograd
    in float64.  PRO: the forward output went through a GELU (pre = its input); XACT: xin = gelu(x); XGRAD: gx is taken
    through gelu'(xg) -- for an XACT layer xg = x (gradient of the pre-activation), otherwise an independent tensor (the
    Fourier layer's pre-activation of the block)."""
    g = torch.Generator().manual_seed(ci + 5 * co + flags)
    B, S = 2, 96
    x = torch.randn(B, ci, S, generator=g)
    w = torch.randn(co, ci, generator=g) / ci ** 0.5
    gout = torch.randn(B, co, S, generator=g)
    skip = torch.randn(B, co, S, generator=g) if gated else None
    gate = torch.randn(co, generator=g) if gated else None
    add = torch.randn(B, ci, S, generator=g) if addend else None
    xg = x if flags & XACT else (torch.randn(B, ci, S, generator=g) if flags & XGRAD else None)
    # float64 reference
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    sd = None if skip is None else skip.double().requires_grad_(True)
    gd = None if gate is None else gate.double().requires_grad_(True)
    xin = F.gelu(xd) if flags & XACT else xd
    z = torch.einsum("oc,bcs->bos", wd, xin)
    if gated:
        z = z + gd[None, :, None] * sd
    out = F.gelu(z) if flags & PRO else z
    out.backward(gout.double())
    pre = z.detach().float().contiguous() if flags & PRO else None      # (einsum may hand back a permuted view)
    gx_ref = xd.grad
    if flags & XGRAD and not flags & XACT:                 # an independent xg: (W^T g + addend) (.) gelu'(xg)
        t = xg.double().requires_grad_(True)
        F.gelu(t).backward(torch.ones_like(t))
        gx_ref = (gx_ref + (0 if add is None else add.double())) * t.grad
    elif flags & XACT:                                     # autograd already went through gelu(x); an addend joins before it
        if add is not None:
            t = x.double().requires_grad_(True)
            F.gelu(t).backward(add.double())
            gx_ref = gx_ref + t.grad
    elif add is not None:
        gx_ref = gx_ref + add.double()
    # engine
    gx, gw, gb = torch.full_like(x, float("nan")), torch.full_like(w, float("nan")), torch.full((co,), float("nan"))
    gsk = torch.full((B, co, S), float("nan")) if gated else None
    ggt = torch.full((co,), float("nan")) if gated else None
    ws = torch.empty(lib.pointwise_linear_workspace_bytes_ex(B, ci, co, S), dtype=torch.uint8)
    lib.pointwise_linear_backward_ex(B, ci, co, S, flags, p(x), p(w), p(gout), p(pre), p(xg), p(skip), p(gate), p(add), p(gx), p(gw),
                                     p(gb), p(gsk), p(ggt), p(ws), 0)
    assert rel_l2(gx.numpy(), gx_ref.numpy()) < TOL
    assert rel_l2(gw.numpy(), wd.grad.numpy()) < TOL
    gz = gout.double()
    if flags & PRO:
        t = z.detach().requires_grad_(True)
        F.gelu(t).backward(gout.double())
        gz = t.grad
    assert rel_l2(gb.numpy(), gz.sum((0, 2)).numpy()) < TOL
    if gated:
        assert rel_l2(gsk.numpy(), sd.grad.numpy()) < TOL and rel_l2(ggt.numpy(), gd.grad.numpy()) < TOL
    # the weight gradients alone (gx = NULL): same bits -- except for the plain map (no option, no gate), which takes the LEAN
    # instantiation on twice the workgroups (another order of the partial sums)
    gw2, gb2 = torch.full_like(w, float("nan")), torch.full((co,), float("nan"))
    ggt2 = torch.full((co,), float("nan")) if gated else None
    lib.pointwise_linear_backward_ex(B, ci, co, S, flags & ~XGRAD, p(x), p(w), p(gout), p(pre), 0, p(skip), p(gate), 0, 0, p(gw2),
                                     p(gb2), 0, p(ggt2), p(ws), 0)
    if (flags & ~XGRAD) == 0 and not gated:
        assert rel_l2(gw2.numpy(), gw.numpy()) < 1e-6 and rel_l2(gb2.numpy(), gb.numpy()) < 1e-6
    else:
        assert torch.equal(gw2, gw) and torch.equal(gb2, gb) and (not gated or torch.equal(ggt2, ggt))


@pytest.mark.parametrize("chans", [(128, 64, 128), (128, 128, 128), (64, 128, 64)], ids=str)
@pytest.mark.parametrize("act", [1, 0])
def test_two_pass_channel_mlp_with_gated_skip(lib, chans, act):
    """fc1, fc2 as two passes each way (what blocks.PointwiseMLP2Fn issues) == autograd of
    act(W2 gelu(W1 x + b1) + b2 + gate (.) skip) in float64"""
    ci, ch, co = chans
    g = torch.Generator().manual_seed(ci + ch + act)
    B, S = 2, 64
    x = torch.randn(B, ci, S, generator=g)
    w1, b1 = torch.randn(ch, ci, generator=g) / ci ** 0.5, torch.randn(ch, generator=g)
    w2, b2 = torch.randn(co, ch, generator=g) / ch ** 0.5, torch.randn(co, generator=g)
    skip, gate, gout = torch.randn(B, co, S, generator=g), torch.randn(co, generator=g), torch.randn(B, co, S, generator=g)
    leaves = [t.double().requires_grad_(True) for t in (x, w1, b1, w2, b2, skip, gate)]
    xd, w1d, b1d, w2d, b2d, sd, gd = leaves
    h = F.gelu(torch.einsum("hc,bcs->bhs", w1d, xd) + b1d[None, :, None])
    z = torch.einsum("oh,bhs->bos", w2d, h) + b2d[None, :, None] + gd[None, :, None] * sd
    ref = F.gelu(z) if act else z
    ref.backward(gout.double())
    hpre, out = torch.empty(B, ch, S), torch.empty(B, co, S)
    zpre = torch.empty(B, co, S) if act else None
    lib.pointwise_linear_forward_ex(B, ci, ch, S, 0, p(x), p(w1), p(b1), 0, 0, p(hpre), 0, 0)
    lib.pointwise_linear_forward_ex(B, ch, co, S, XACT | (ACT if act else 0), p(hpre), p(w2), p(b2), p(skip), p(gate), p(out), p(zpre), 0)
    assert rel_l2(out.numpy(), ref.detach().numpy()) < TOL
    ghp, gx = torch.empty_like(hpre), torch.empty_like(x)
    gw1, gw2, gb1, gb2 = torch.empty_like(w1), torch.empty_like(w2), torch.empty_like(b1), torch.empty_like(b2)
    gsk, ggt = torch.empty_like(skip), torch.empty_like(gate)
    ws = torch.empty(max(lib.pointwise_linear_workspace_bytes_ex(B, ch, co, S), lib.pointwise_linear_workspace_bytes_ex(B, ci, ch, S)),
                     dtype=torch.uint8)
    lib.pointwise_linear_backward_ex(B, ch, co, S, XACT | XGRAD | (PRO if act else 0), p(hpre), p(w2), p(gout), p(zpre), p(hpre),
                                     p(skip), p(gate), 0, p(ghp), p(gw2), p(gb2), p(gsk), p(ggt), p(ws), 0)
    lib.pointwise_linear_backward_ex(B, ci, ch, S, 0, p(x), p(w1), p(ghp), 0, 0, 0, 0, 0, p(gx), p(gw1), p(gb1), 0, 0, p(ws), 0)
    for got, want in zip((gx, gw1, gb1, gw2, gb2, gsk, ggt), leaves):
        assert rel_l2(got.numpy(), want.grad.numpy()) < TOL


def test_argument_checks(lib):
    x, w, out = torch.zeros(1, 64, 32), torch.zeros(128, 64), torch.zeros(1, 128, 32)
    with pytest.raises(_lib.EngineError):                # 48 channels
        lib.pointwise_linear_forward_ex(1, 48, 128, 32, 0, p(x), p(w), 0, 0, 0, p(out), 0, 0)
    with pytest.raises(_lib.EngineError):                # spatial not a multiple of 32
        lib.pointwise_linear_forward_ex(1, 64, 128, 40, 0, p(x), p(w), 0, 0, 0, p(out), 0, 0)
    with pytest.raises(_lib.EngineError):                # 2^28 points per image: lane offsets are 32-bit byte counts (no launch)
        lib.pointwise_linear_forward_ex(1, 64, 128, 1 << 28, 0, p(x), p(w), 0, 0, 0, p(out), 0, 0)
    with pytest.raises(_lib.EngineError):                # a gate without its source
        lib.pointwise_linear_forward_ex(1, 64, 128, 32, 0, p(x), p(w), 0, 0, p(w), p(out), 0, 0)
    with pytest.raises(_lib.EngineError):                # a backward flag in a forward call
        lib.pointwise_linear_forward_ex(1, 64, 128, 32, PRO, p(x), p(w), 0, 0, 0, p(out), 0, 0)
    ws = torch.empty(lib.pointwise_linear_workspace_bytes_ex(1, 64, 128, 32), dtype=torch.uint8)
    with pytest.raises(_lib.EngineError):                # PRO without the pre-activation
        lib.pointwise_linear_backward_ex(1, 64, 128, 32, PRO, p(x), p(w), p(out), 0, 0, 0, 0, 0, p(x), p(w), 0, 0, 0, p(ws), 0)
    assert lib.pointwise_linear_workspace_bytes_ex(1, 48, 64, 32) == 0


# ---- the kernel-edge tables of tests/pointwise_reference.py at the tile counts the emulated chip takes ---------------------
EMU_A = [(kind, name) for kind in ("plinx_fwd", "plinx_bwd")
         for name in pr.emu_subset(pr.TABLES[kind], lambda c: (c["ci"], c["co"], pr.instantiation("plinx_bwd", dict(c, want_gx=c.get("want_gx", 1)))))]


@pytest.mark.parametrize("kind,name", EMU_A, ids=[f"{k}-{n}" for k, n in EMU_A])
def test_tile_placement_inside_guard_bands(lib, kind, name):
    """Table A at T <= 15 for every channel pair (and the LEAN instantiation): guard bands, per-element bounds, rel-L2.
    One compute unit: k_plinx_fwd has 2 workgroups, k_plinx_bwd 1 or 2 -- T = 15 loops them"""
    cfg = pr.TABLES[kind][name]
    pr.run_case(kind, lib, cfg, guard=True, seed=11)


LOOP_KINDS = [("plinx_fwd", dict(ci=ci, co=co, flags=XACT | ACT, gated=True, pre_out=1)) for ci, co in ((32, 32), (64, 128), (128, 128))]
LOOP_KINDS += [("plinx_bwd", dict(ci=ci, co=co, flags=XACT | XGRAD | PRO, gated=True, addend=True, want_gx=1))
               for ci, co in ((32, 32), (64, 128), (128, 128))]
LOOP_KINDS += [("plinx_bwd", dict(ci=ci, co=co, flags=0, gated=False, addend=False, want_gx=0)) for ci, co in ((64, 64), (128, 128))]


@pytest.mark.parametrize("kind,cfg", LOOP_KINDS, ids=[f"{k}-{c['ci']}_{c['co']}-gx{c.get('want_gx', '')}" for k, c in LOOP_KINDS])
def test_nine_tiles_loop_on_one_compute_unit(lib, kind, cfg):
    """the caps follow sc_cu_count() = 1 here (4 or 8 tiles per round): T = 9 is two or three rounds, the last ragged; for
    the backward pass also with gout zero outside the last tile, tile 0 and the last tile of the first round"""
    cap = pr.cap_of(kind, cfg, 1)
    cfg = pr.with_tiles(cfg, 9)
    assert 9 > 4 * cap
    pr.run_case(kind, lib, cfg, seed=7, expect_n_wg=cap)
    if kind == "plinx_bwd":
        for tile in (8, 0, 4 * cap - 1):
            got, _, _ = pr.run_case(kind, lib, cfg, seed=7, mark=tile, expect_n_wg=cap)
            pr.assert_zero_outside_tile(got, cfg, tile)


@pytest.mark.parametrize("tiles", [1, 9])
def test_two_launches_share_one_partial_buffer_at_128_to_128(lib, tiles):
    """om0 = 0 and 2: the second launch's final stage writes rows 64.. of gw / gb / ggate and leaves rows 0..63 alone"""
    cfg = pr.with_tiles(dict(ci=128, co=128, flags=PRO, gated=True, addend=False, want_gx=1), tiles)
    pr.run_case("plinx_bwd", lib, cfg, guard=True, seed=19, expect_n_wg=1)
