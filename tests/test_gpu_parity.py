"""GPU tier (``-m gpu``): the HIP engine, called through the C-ABI, against
(a) the golden vectors of the verbatim reference, (b) the CPU oracle on seeded inputs at
sizes the oracle finishes in seconds, (c) size-independent properties at the BASELINE
metric shape.  Parity bar: rel-L2 <= 1e-5 in fp32 (north star)."""
import numpy as np
import pytest
import torch

from conftest import DENSE_GOLDEN, FACT_GOLDEN, golden_names, load_golden
from engine_runner import layer_fwd_bwd, rel_l2

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def lib():
    from neuraloperator_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("GPU tier: no GPU visible")            # selected by hand on a CPU box; the driver runs -m gpu on MI355X
    return _lib.get_lib()      # raises if libsc_engine.so is missing: no fallback


@pytest.mark.parametrize("flags", [0, 1, 5], ids=["default", "force_generic", "force_generic_valu"])
@pytest.mark.parametrize("name", DENSE_GOLDEN)
def test_golden(lib, name, flags):
    g = load_golden(name)
    dev = torch.device("cuda:0")
    x, w, b, gy = (torch.from_numpy(g[k]).to(dev) for k in ("x", "weight", "bias", "g"))
    y, gx, gw, gb, _ = layer_fwd_bwd(lib, x, w, b, gy, list(g["n_modes_attr"]),
                                     list(g["max_n_modes_attr"]), flags=flags)
    assert rel_l2(y.cpu().numpy(), g["y"]) < TOL
    assert rel_l2(gx.cpu().numpy(), g["gx"]) < TOL
    assert rel_l2(gw.cpu().numpy(), g["gw"]) < TOL
    assert rel_l2(gb.cpu().numpy(), g["gbias"]) < TOL


ORACLE_CASES = [
    # B, Cin, Cout, spatial, n_modes, max_n_modes
    (2, 16, 16, (128, 128), (32, 32), None),
    (2, 64, 64, (256, 256), (64, 64), None),        # BASELINE metric shape, reduced batch
    (3, 5, 7, (100, 60), (20, 14), None),           # non power of two, ragged channels
    (2, 8, 8, (64, 64), (16, 16), (32, 32)),        # centred sub-block of a larger weight
    (2, 8, 8, (32, 32, 32), (8, 8, 8), None),
    (1, 4, 4, (64, 64, 64), (16, 16, 16), None),
    (4, 6, 6, (512,), (64,), None),
    (1, 3, 3, (9, 11, 8), (5, 7, 4), None),
    (2, 4, 4, (256, 256), (256, 256), None),        # keep everything
    (2, 3, 5, (40, 128), (8, 32), None),            # kept 8 x 17: matrix-core pass with the VALU tail column
    (2, 3, 5, (20, 72), (8, 64), None),             # ... kept 8 x 33, width not a multiple of 32
    (1, 4, 4, (16, 128, 128), (8, 32, 32), None),   # 128-row second-to-last axis: last two axes in one launch
    (2, 4, 4, (128, 64), (40, 16), None),           # ... 40 kept rows = 4 row tiles (3 used)
    (32, 64, 64, (32, 32), (16, 16), None),         # channel counts that take the MFMA contraction
    (64, 64, 64, (24, 20), (8, 10), None),          # ... with P = 64 row tiles in forward, odd-ish grid
    (32, 64, 64, (32, 32), (12, 12), (16, 16)),     # ... through the sub-block index tables
    (8, 32, 32, (32, 32, 32), (16, 16, 16), None),  # small batch: gX-hat streams with clamped rows, backward pair launch
    (12, 32, 48, (64, 64), (32, 30), None),         # ... 12 rows, ragged second column tile (kept 32 x 16)
    # round 4: the reference's Darcy grids (85 / 141 / 211 / 421 points, not multiples of 8) on the matrix cores
    # (k_mdft_r2c<.., RAGGED>, per-row bias lookup in k_mdft_c2r: image heights are odd)
    (2, 4, 4, (85, 85), (32, 32), None),
    (2, 3, 5, (141, 141), (64, 64), None),
    (1, 4, 4, (211, 211), (32, 32), None),
    (1, 2, 3, (421, 421), (32, 32), None),
    (2, 3, 3, (9, 11, 43), (4, 6, 16), None),
    (2, 3, 3, (70, 601), (8, 32), None),            # ... a 77 KB span image (dynamic LDS past 64 KB), 3 partial blocks
    (1, 2, 2, (40, 701), (8, 32), None),            # ... a span that does not fit: the 128-line chunked inverse kernel
    # round 3: two-pass factorised route for lines of 32 P points, P in {2, 3, 4, 5, 6, 8, 10, 12, 20}
    (2, 8, 8, (64, 64), (32, 32), None),            # P = 2
    (2, 4, 6, (96, 96), (24, 24), None),            # P = 3
    (2, 8, 8, (192, 192), (64, 64), None),          # P = 6
    (1, 4, 4, (384, 640), (48, 48), None),          # P = 12, 20
    (2, 3, 5, (160, 320), (20, 20), None),          # P = 5, 10
    (1, 4, 4, (256, 256), (128, 128), None),        # P = 8: kept block beyond the fused kernels' 64 x 33
]


def _oracle_layer(x, w, bias, g, nm, contract=None):
    """The CPU oracle (spectral_convolution.py:417-570 restated + autograd) on host copies of device tensors:
    returns (y, gx, gW or None, gbias) as numpy arrays.  Used by the multi-GPU-layer / fused-block tests so that they
    compare the HIP path with the ORACLE, not with another HIP path."""
    from oracle import spectral_oracle as so
    xc = x.detach().cpu().clone().requires_grad_(True)
    wc = w.detach().cpu().clone().requires_grad_(contract is None)
    bc = bias.detach().cpu().clone().requires_grad_(True)
    kw = {} if contract is None else dict(contract=contract)
    yo = so.forward_torch(xc, wc, bc, list(nm), list(nm), **kw)
    yo.backward(g.detach().cpu())
    return (yo.detach().numpy(), xc.grad.numpy(), None if wc.grad is None else wc.grad.numpy(), bc.grad.numpy())


def _bf16_checks(y, y_ref32, what):
    """bfloat16 result against the fp32 oracle on the same (bf16-valued) inputs: the engine rounds its fp32
    result once (nearest even), so it is within one bf16 ulp of the oracle and bit-identical to the rounded
    oracle except where the two fp32 values straddle a rounding boundary."""
    assert y.dtype == torch.bfloat16, what
    y, y_ref32 = y.cpu(), y_ref32.cpu()
    err = (y.float() - y_ref32).abs()
    bound = y_ref32.abs() * 2.0 ** -8 + 1e-5 * y_ref32.abs().max()
    assert bool((err <= bound).all()), f"{what}: {float((err - bound).max())} past one bf16 ulp"
    same = (y.view(torch.int16) == y_ref32.bfloat16().view(torch.int16)).float().mean().item()
    assert same > 0.98, f"{what}: only {same:.4f} of the values equal the rounded oracle bit for bit"


@pytest.mark.parametrize("case", [(2, 16, 16, 256, (64, 64)), (3, 4, 6, 64, (20, 16)), (2, 8, 8, 512, (64, 64)),
                                  (32, 64, 64, 128, (32, 32))],
                         ids=lambda c: f"H{c[3]}_m{c[4][0]}_c{c[1]}")
def test_bf16_io_vs_oracle(lib, case):
    """SC_PLAN_IO_BF16 through the C-ABI (BASELINE configs[1] "bf16"): x / gy are bfloat16 in HBM, y / gx are
    stored as bfloat16, spectra / weights / their gradients and all arithmetic stay fp32."""
    from oracle import spectral_oracle as so
    from neuraloperator_amd import _lib
    from neuraloperator_amd.modes import halve_last_mode

    b, ci, co, H, modes = case
    torch.manual_seed(77)
    nm = halve_last_mode(modes)
    std = (2 / (ci + co)) ** 0.5
    x = torch.randn(b, ci, H, 256).bfloat16()
    w = torch.empty(ci, co, *nm, dtype=torch.cfloat).normal_(0, std)
    bias = std * torch.randn(co, 1, 1)
    g = torch.randn(b, co, H, 256).bfloat16()
    xc, wc, bc = x.float().requires_grad_(True), w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    yo = so.forward_torch(xc, wc, bc, nm, nm)
    yo.backward(g.float())
    dev = torch.device("cuda:0")
    y, gx, gw, gb, xh = layer_fwd_bwd(lib, x.to(dev), w.to(dev), bias.to(dev), g.to(dev), nm, nm,
                                      flags=_lib.SC_PLAN_IO_BF16)
    _bf16_checks(y, yo.detach(), "y")
    _bf16_checks(gx, xc.grad, "gx")
    assert rel_l2(gw.cpu().numpy(), wc.grad.numpy()) < TOL
    assert rel_l2(gb.cpu().numpy(), bc.grad.numpy()) < TOL
    # the fp32-I/O kernels on the same values: the same fp32 spectrum bit for bit from the vector-ALU kernel (same
    # arithmetic; SC_PLAN_NO_MX_FFT, and H = 512 always), fp32 round-off apart from the matrix-core row pass (round 5:
    # k_fft2d_fwd_mx -- the bf16 input is exact in the MFMA's input format; round 6: the twiddles are TWO bf16 terms by
    # default (spectrum 1.3e-6 away: 3000 x below the input's own 2^-9, 8 x below TOL of the gradients checked above), three
    # with SC_PLAN_MX_FFT_3TERM (fp32 round-off class))
    _, _, _, _, xh32 = layer_fwd_bwd(lib, x.float().to(dev), w.to(dev), bias.to(dev), g.float().to(dev), nm, nm)
    _, _, _, _, xh3 = layer_fwd_bwd(lib, x.to(dev), w.to(dev), bias.to(dev), g.to(dev), nm, nm,
                                    flags=_lib.SC_PLAN_IO_BF16 | _lib.SC_PLAN_MX_FFT_3TERM)
    _, _, _, _, xhv = layer_fwd_bwd(lib, x.to(dev), w.to(dev), bias.to(dev), g.to(dev), nm, nm,
                                    flags=_lib.SC_PLAN_IO_BF16 | _lib.SC_PLAN_NO_MX_FFT)
    assert torch.equal(xhv, xh32)
    if H == 512:
        assert torch.equal(xh, xh32) and torch.equal(xh3, xh32)
    else:
        assert rel_l2(xh.cpu().numpy(), xh32.cpu().numpy()) < 3e-6
        assert rel_l2(xh3.cpu().numpy(), xh32.cpu().numpy()) < 1e-6


@pytest.mark.parametrize("H", [64, 128, 256])
def test_bf16_inverse_on_the_matrix_cores_is_repeatable_and_one_rounding_from_fp32(lib, H):
    """k_fft2d_inv_mx (round 5, session 2: the row pass of the inverse-type transform writing bfloat16 as bf16 MFMA
    products, two terms per operand) at the metric's image count: thirty launches bit for bit the same, within one bf16
    ulp of the vector-ALU kernel everywhere and different from it on < 1 % of the outputs, both inverse-type modes.
    H = 64 since round 6: round 5's build of that height was not repeatable on hardware -- a packed-fp32 instruction with
    op_sel:[0,1] beside the other workgroup's bf16 MFMAs (tests/test_isa_pk_forms.py guards the encoding,
    scripts/mx_ifft_repeat.py is the long soak)."""
    from neuraloperator_amd import _lib

    dev = torch.device("cuda:0")
    torch.manual_seed(21)
    n, C = 2048, 64
    yh = torch.randn(n, 64, 33, 2, device=dev)
    bias = torch.randn(C, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    pm = lib.plan_create([H, 256], [64, 33], flags=_lib.SC_PLAN_IO_BF16)
    pv = lib.plan_create([H, 256], [64, 33], flags=_lib.SC_PLAN_IO_BF16 | _lib.SC_PLAN_NO_MX_FFT)
    assert lib.plan_kernel_name(pm, 1) == "k_fft2d_inv_mx" and lib.plan_kernel_name(pv, 1) == "k_fft2d_inv3"
    for mode, b in ((_lib.SC_INV_PADDED, bias.data_ptr()), (_lib.SC_INV_ADJ_R2C, 0)):
        y0 = torch.zeros(n, H, 256, device=dev, dtype=torch.bfloat16)
        yv, y = torch.zeros_like(y0), torch.zeros_like(y0)
        lib.transform_inverse(pm, mode, yh.data_ptr(), b, C, y0.data_ptr(), n, 0, st)
        lib.transform_inverse(pv, mode, yh.data_ptr(), b, C, yv.data_ptr(), n, 0, st)
        for _ in range(30 if mode == _lib.SC_INV_PADDED else 10):
            lib.transform_inverse(pm, mode, yh.data_ptr(), b, C, y.data_ptr(), n, 0, st)
            assert torch.equal(y.view(torch.int16), y0.view(torch.int16))
        d = (y0.float() - yv.float()).abs()
        assert bool((d <= yv.float().abs() * 2.0 ** -7 + 1e-4 * yv.float().abs().max()).all())
        assert float((y0 != yv).float().mean()) < 0.01
    lib.plan_destroy(pm)
    lib.plan_destroy(pv)


def test_bf16_forward_on_a_4_byte_aligned_view(lib):
    """k_fft2d_fwd_mx (round 5) loads whole rows 16 bytes per lane: a bf16 tensor that starts 4 bytes into an allocation
    (legal for the vector-ALU kernel's 4-byte accesses) takes k_fft2d_fwd3 -- same bits as a plan with
    SC_PLAN_NO_MX_FFT; the aligned tensor takes the matrix-core kernel, fp32 round-off away."""
    from neuraloperator_amd import _lib

    dev = torch.device("cuda:0")
    torch.manual_seed(8)
    n, H = 6, 128
    flat = torch.randn(n * H * 256 + 8, device=dev).bfloat16()
    x_odd = flat[2:2 + n * H * 256].view(n, H, 256)
    assert x_odd.data_ptr() % 16 == 4
    x_al = x_odd.clone()
    assert x_al.data_ptr() % 16 == 0
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for tag, fl, xin in (("mx_aligned", _lib.SC_PLAN_IO_BF16, x_al), ("mx_odd", _lib.SC_PLAN_IO_BF16, x_odd),
                         ("valu", _lib.SC_PLAN_IO_BF16 | _lib.SC_PLAN_NO_MX_FFT, x_al)):
        plan = lib.plan_create([H, 256], [64, 33], flags=fl)
        xh = torch.zeros(n, 64, 33, 2, device=dev)
        lib.transform_forward(plan, _lib.SC_FWD_SCALED, xin.data_ptr(), xh.data_ptr(), n, 0, st)
        torch.cuda.synchronize()
        out[tag] = xh
        lib.plan_destroy(plan)
    assert torch.equal(out["mx_odd"], out["valu"])
    assert not torch.equal(out["mx_aligned"], out["valu"])
    assert rel_l2(out["mx_aligned"].cpu().numpy(), out["valu"].cpu().numpy()) < 3e-6      # two-term twiddles (round 6 default)


def test_module_bf16_activations():
    """bfloat16 in -> bfloat16 out through the drop-in module: native bf16 I/O on the fused kernels, conversion
    around the fp32 engine everywhere else; gradients arrive in the dtypes autograd expects."""
    from neuraloperator_amd import SpectralConv, engine

    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    for spatial, modes, native in [((64, 256), (16, 16), True), ((48, 40), (12, 12), False)]:
        conv = SpectralConv(6, 5, modes).to(dev)
        x = torch.randn(2, 6, *spatial, device=dev).bfloat16().requires_grad_(True)
        g = torch.randn(2, 5, *spatial, device=dev).bfloat16()
        y = conv(x)
        assert y.dtype == torch.bfloat16
        y.backward(g)
        assert x.grad.dtype == torch.bfloat16 and conv.weight.tensor.grad.dtype == torch.complex64
        gw, gb = conv.weight.tensor.grad.clone(), conv.bias.grad.clone()
        kept = [modes[0], modes[1] // 2 + 1]
        assert (engine.get_plan_bf16_io(dev, list(spatial), kept, "forward", 0) is not None) == native
        # the same module on the fp32 copies of the same values
        conv.zero_grad()
        x32 = x.detach().float().requires_grad_(True)
        y32 = conv(x32)
        y32.backward(g.float())
        _bf16_checks(y.detach(), y32.detach(), "y")
        _bf16_checks(x.grad, x32.grad, "gx")
        assert rel_l2(gw.cpu().numpy(), conv.weight.tensor.grad.cpu().numpy()) < TOL
        assert rel_l2(gb.cpu().numpy(), conv.bias.grad.cpu().numpy()) < TOL


@pytest.mark.parametrize("flags", [0, 1, 5, 64], ids=["default", "force_generic", "force_generic_valu", "two_pass_small"])
@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: "x".join(map(str, c[3])) + f"_m{c[4][0]}_c{c[1]}")
def test_vs_oracle(lib, case, flags):
    from oracle import spectral_oracle as so
    from neuraloperator_amd.modes import halve_last_mode

    b, ci, co, spatial, modes, maxm = case
    torch.manual_seed(1234)
    nm = halve_last_mode(modes)
    mx = halve_last_mode(maxm) if maxm is not None else list(nm)
    std = (2 / (ci + co)) ** 0.5
    x = torch.randn(b, ci, *spatial)
    w = torch.empty(ci, co, *mx, dtype=torch.cfloat).normal_(0, std)
    bias = std * torch.randn(co, *(1,) * len(spatial))
    g = torch.randn(b, co, *spatial)
    xc, wc, bc = x.clone().requires_grad_(True), w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    yo = so.forward_torch(xc, wc, bc, nm, mx)
    yo.backward(g)
    dev = torch.device("cuda:0")
    y, gx, gw, gb, _ = layer_fwd_bwd(lib, x.to(dev), w.to(dev), bias.to(dev), g.to(dev), nm, mx, flags=flags)
    assert rel_l2(y.cpu().numpy(), yo.detach().numpy()) < TOL
    assert rel_l2(gx.cpu().numpy(), xc.grad.numpy()) < TOL
    assert rel_l2(gw.cpu().numpy(), wc.grad.numpy()) < TOL
    assert rel_l2(gb.cpu().numpy(), bc.grad.numpy()) < TOL


DARCY_CASES = [c for c in ORACLE_CASES if c[3] in ((85, 85), (141, 141), (211, 211), (421, 421), (9, 11, 43))]


@pytest.mark.parametrize("case", DARCY_CASES, ids=lambda c: "x".join(map(str, c[3])) + f"_m{c[4][0]}")
def test_odd_widths_chunked_inverse_vs_oracle(lib, case):
    """SC_PLAN_NO_SPAN: the inverse last-axis pass of the odd grids through the 128-line chunked kernel
    (k_mdft_c2r_stage) instead of the 32-line whole-span one -- the kernel that runs when a tensor is not 16-byte
    aligned or its span does not fit LDS; and the same layer on a view with an odd storage offset."""
    from oracle import spectral_oracle as so
    from neuraloperator_amd.modes import halve_last_mode
    from neuraloperator_amd import _lib

    b, ci, co, spatial, modes, _ = case
    torch.manual_seed(4321)
    nm = halve_last_mode(modes)
    std = (2 / (ci + co)) ** 0.5
    x = torch.randn(b, ci, *spatial)
    w = torch.empty(ci, co, *nm, dtype=torch.cfloat).normal_(0, std)
    bias = std * torch.randn(co, *(1,) * len(spatial))
    g = torch.randn(b, co, *spatial)
    xc, wc, bc = x.clone().requires_grad_(True), w.clone().requires_grad_(True), bias.clone().requires_grad_(True)
    yo = so.forward_torch(xc, wc, bc, nm, nm)
    yo.backward(g)
    dev = torch.device("cuda:0")
    plan = lib.plan_create(list(spatial), list(nm), flags=_lib.SC_PLAN_NO_SPAN)
    assert lib.plan_kernel_name(plan, 1) == "k_mdft_c2r_stage"
    lib.plan_destroy(plan)
    xd = x.to(dev)
    buf = torch.zeros(x.numel() + 1, device=dev)
    x_odd = buf[1:].view_as(x).copy_(xd)                       # 4-byte aligned only
    for xin, flags in ((xd, _lib.SC_PLAN_NO_SPAN), (x_odd, 0)):
        y, gx, gw, gb, _ = layer_fwd_bwd(lib, xin, w.to(dev), bias.to(dev), g.to(dev), nm, nm, flags=flags)
        assert rel_l2(y.cpu().numpy(), yo.detach().numpy()) < TOL
        assert rel_l2(gx.cpu().numpy(), xc.grad.numpy()) < TOL
        assert rel_l2(gw.cpu().numpy(), wc.grad.numpy()) < TOL
        assert rel_l2(gb.cpu().numpy(), bc.grad.numpy()) < TOL


@pytest.mark.parametrize("spatial,kept", [((64, 64), (32, 17)), ((96, 96), (24, 13)), ((192, 192), (64, 33)),
                                          ((384, 640), (48, 25)), ((256, 256), (128, 65)), ((160, 320), (20, 11))])
def test_factorised_route_for_32p_lines(lib, spatial, kept):
    """Round 3: grids of 32 P points per axis (64 .. 640) are never on the direct-DFT passes any more; the fused
    256-wide kernels and the 128 x 128 plane kernels keep their shapes."""
    from neuraloperator_amd import _lib as L
    small = spatial[0] * spatial[1] < 128 * 128          # small planes: the one-launch direct-DFT passes are faster
    plan = lib.plan_create(list(spatial), list(kept))
    try:
        name = lib.plan_kernel_name(plan, 0)
        if spatial == (64, 64):                          # session 2: its own one-launch plane kernels (sc_kernels_plane64.h)
            assert name == "k_pl64_fwd" and lib.plan_kernel_name(plan, 1) == "k_pl64_inv"
        else:
            assert (name != "k_f2p_r2c") if small else (name == "k_f2p_r2c" and lib.plan_kernel_name(plan, 1) == "k_f2p_c2r")
    finally:
        lib.plan_destroy(plan)
    plan = lib.plan_create(list(spatial), list(kept), flags=L.SC_PLAN_F2P_SMALL_ALWAYS)
    try:
        assert lib.plan_kernel_name(plan, 0) == "k_f2p_r2c" and lib.plan_kernel_name(plan, 1) == "k_f2p_c2r"
    finally:
        lib.plan_destroy(plan)
    plan = lib.plan_create(list(spatial), list(kept), flags=L.SC_PLAN_NO_F2P_SMALL)
    try:
        assert lib.plan_kernel_name(plan, 0) != "k_f2p_r2c"
    finally:
        lib.plan_destroy(plan)
    for sp, kp, name in (((256, 256), (64, 33), "k_fft2d_fwd3"), ((128, 128), (32, 17), "k_pl128_fwd")):
        plan = lib.plan_create(list(sp), list(kp))
        try:
            assert lib.plan_kernel_name(plan, 0) == name
        finally:
            lib.plan_destroy(plan)


def test_full_size_properties(lib):
    """BASELINE metric shape at full size (B=32, C=64, 256^2, modes 64): linearity in x,
    adjointness <y, g> == <x, gx> == Re<W, gW>, bias grad, and fp64 known-answer spot checks."""
    from neuraloperator_amd.modes import halve_last_mode

    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    b, c, n, m = 32, 64, 256, 64
    nm = halve_last_mode((m, m))
    std = (2 / (2 * c)) ** 0.5
    x1 = torch.randn(b, c, n, n, device=dev)
    x2 = torch.randn(b, c, n, n, device=dev)
    w = torch.empty(c, c, *nm, dtype=torch.cfloat, device=dev).normal_(0, std)
    zero_b = torch.zeros(c, 1, 1, device=dev)
    g = torch.randn(b, c, n, n, device=dev)
    y1, gx1, gw1, gb1, xh1 = layer_fwd_bwd(lib, x1, w, zero_b, g, nm, nm)
    y2, _, gw2, _, _ = layer_fwd_bwd(lib, x2, w, zero_b, g, nm, nm)
    y12, _, gw12, _, _ = layer_fwd_bwd(lib, x1 + 2 * x2, w, zero_b, g, nm, nm)
    # linearity of the forward map and of gW in x
    assert rel_l2((y1 + 2 * y2).cpu().numpy(), y12.cpu().numpy()) < TOL
    assert rel_l2((gw1 + 2 * gw2).cpu().numpy(), gw12.cpu().numpy()) < TOL
    # adjointness: <conv(x1), g> == <x1, gx>   (bias = 0; fp64 accumulation)
    lhs = (y1.double() * g.double()).sum().item()
    rhs = (x1.double() * gx1.double()).sum().item()
    assert abs(lhs - rhs) / max(abs(lhs), 1e-30) < 1e-4
    # <y, g> is also Re <W, gW> summed over the weight (y linear in W)
    rhs_w = (w.conj().to(torch.complex128) * gw1.to(torch.complex128)).real.sum().item()
    assert abs(lhs - rhs_w) / max(abs(lhs), 1e-30) < 1e-4
    # bias gradient is the plain sum of g
    assert rel_l2(gb1.cpu().numpy().ravel(), g.double().sum(dim=(0, 2, 3)).float().cpu().numpy()) < TOL
    # known-answer spot checks in fp64: a few kept coefficients of xhat straight from the DFT sum,
    # and a few output pixels from the zero-padded inverse sum over yhat = einsum(xhat, W)
    gen = torch.Generator().manual_seed(0)
    hh = torch.arange(n, device=dev, dtype=torch.float64)
    for _ in range(6):
        bi, ci = int(torch.randint(b, (1,), generator=gen)), int(torch.randint(c, (1,), generator=gen))
        r, col = int(torch.randint(nm[0], (1,), generator=gen)), int(torch.randint(nm[1], (1,), generator=gen))
        fx, fy = r - nm[0] // 2, col
        ph = torch.exp(-2j * torch.pi * (fx * hh[:, None] / n + fy * hh[None, :] / n))
        want = (x1[bi, ci].double() * ph).sum() / (n * n)
        got = xh1[bi, ci, r, col].to(torch.complex128)
        assert abs(got - want) / abs(want) < 1e-4
    yhat = torch.einsum("bixy,ioxy->boxy", xh1.to(torch.complex128), w.to(torch.complex128))
    fxs = (torch.arange(nm[0], device=dev) - nm[0] // 2).double()
    fys = torch.arange(nm[1], device=dev).double()
    cw = torch.full((nm[1],), 2.0, device=dev, dtype=torch.float64)
    cw[0] = 1.0
    for _ in range(6):
        bi, oi = int(torch.randint(b, (1,), generator=gen)), int(torch.randint(c, (1,), generator=gen))
        h0, w0 = int(torch.randint(n, (1,), generator=gen)), int(torch.randint(n, (1,), generator=gen))
        ph = torch.exp(2j * torch.pi * (fxs[:, None] * h0 / n + fys[None, :] * w0 / n))
        col = (yhat[bi, oi] * ph).sum(dim=0)              # inverse along rows first; C2R then takes
        want = (cw * col.real).sum().item()                # c_k * Re(.) (Im of the DC column drops out)
        got = y1[bi, oi, h0, w0].item()
        assert abs(got - want) < 1e-4 * max(1.0, abs(want))


def test_mfma_contractions_full_size(lib):
    """The three contractions of the layer at the BASELINE metric shape (2112 modes, B=32, C=64)
    on the matrix-core kernel vs a complex128 einsum and vs the VALU kernel."""
    from neuraloperator_amd import _lib as L
    dev = torch.device("cuda:0")
    torch.manual_seed(21)
    B, C, M = 32, 64, 64 * 33
    xh = torch.randn(B, C, M, dtype=torch.cfloat, device=dev)
    gh = torch.randn(B, C, M, dtype=torch.cfloat, device=dev)
    w = torch.randn(C, C, M, dtype=torch.cfloat, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def run(a, b, out, flags, **kw):
        assert lib.modegemm_uses_matrix_cores(flags=flags, **kw) == (flags == 0)
        lib.modegemm(torch.view_as_real(a).data_ptr(), torch.view_as_real(b).data_ptr(),
                     torch.view_as_real(out).data_ptr(), st, flags=flags, **kw)
        torch.cuda.synchronize()
        return out

    cases = {
        "fwd": (xh, w, (B, C, M), "bim,iom->bom", dict(P=B, Q=C, R=C, n_modes=M, a_sp=C * M, a_sr=M, a_sm=1,
                b_sr=C * M, b_sq=M, b_sm=1, c_sp=C * M, c_sq=M, c_sm=1), (False, False)),
        "gx": (gh, w, (B, C, M), "bom,iom->bim", dict(P=B, Q=C, R=C, n_modes=M, a_sp=C * M, a_sr=M, a_sm=1,
               b_sr=M, b_sq=C * M, b_sm=1, conj_b=1, c_sp=C * M, c_sq=M, c_sm=1), (False, True)),
        "gw": (xh, gh, (C, C, M), "bim,bom->iom", dict(P=C, Q=C, R=B, n_modes=M, a_sp=M, a_sr=C * M, a_sm=1,
               conj_a=1, b_sr=C * M, b_sq=M, b_sm=1, c_sp=C * M, c_sq=M, c_sm=1), (True, False)),
    }
    for name, (a, b, shape, eq, kw, (ca, cb)) in cases.items():
        a128, b128 = a.to(torch.complex128), b.to(torch.complex128)
        ref = torch.einsum(eq, a128.conj() if ca else a128, b128.conj() if cb else b128).cpu().numpy()
        out = run(a, b, torch.full(shape, float("nan"), dtype=torch.cfloat, device=dev), 0, **kw)
        assert rel_l2(out.cpu().numpy(), ref) < TOL, name
        out2 = run(a, b, torch.empty(shape, dtype=torch.cfloat, device=dev), L.SC_GEMM_FORCE_VALU, **kw)
        assert rel_l2(out2.cpu().numpy(), ref) < TOL, name


def test_small_batch_contractions_full_width(lib):
    """k_modegemm_sb (round 3: a batch of <= 4 rows against a hidden-128 weight, BASELINE configs[4]'s three
    contractions; 8 256 of its 33 024 modes so that the complex128 reference stays small) vs a complex128 einsum and,
    bit for bit, vs the lanes-are-modes VALU kernel it replaces."""
    from neuraloperator_amd import _lib as L
    dev = torch.device("cuda:0")
    torch.manual_seed(22)
    B, C, M = 4, 128, 8256                          # 16 mode tiles of 512 + a ragged one
    xh = torch.randn(B, C, M, dtype=torch.cfloat, device=dev)
    gh = torch.randn(B, C, M, dtype=torch.cfloat, device=dev)
    w = torch.randn(C, C, M, dtype=torch.cfloat, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    cases = {
        "fwd": (xh, w, (B, C, M), "bim,iom->bom", dict(P=B, Q=C, R=C, n_modes=M, a_sp=C * M, a_sr=M, a_sm=1,
                b_sr=C * M, b_sq=M, b_sm=1, c_sp=C * M, c_sq=M, c_sm=1), (False, False)),
        "gx": (gh, w, (B, C, M), "bom,iom->bim", dict(P=B, Q=C, R=C, n_modes=M, a_sp=C * M, a_sr=M, a_sm=1,
               b_sr=M, b_sq=C * M, b_sm=1, conj_b=1, c_sp=C * M, c_sq=M, c_sm=1), (False, True)),
        "gw": (xh, gh, (C, C, M), "bim,bom->iom", dict(P=C, Q=C, R=B, n_modes=M, a_sp=M, a_sr=C * M, a_sm=1,
               conj_a=1, b_sr=C * M, b_sq=M, b_sm=1, c_sp=C * M, c_sq=M, c_sm=1, flags=L.SC_GEMM_STREAM_C),
               (True, False)),
    }
    for name, (a, b, shape, eq, kw, (ca, cb)) in cases.items():
        assert lib.modegemm_path(**kw) == 3, name
        a128, b128 = a.to(torch.complex128), b.to(torch.complex128)
        ref = torch.einsum(eq, a128.conj() if ca else a128, b128.conj() if cb else b128).cpu().numpy()
        out = torch.full(shape, float("nan"), dtype=torch.cfloat, device=dev)
        lib.modegemm(torch.view_as_real(a).data_ptr(), torch.view_as_real(b).data_ptr(),
                     torch.view_as_real(out).data_ptr(), st, **kw)
        kw0 = dict(kw, flags=L.SC_GEMM_NO_SB | L.SC_GEMM_FORCE_VALU | L.SC_GEMM_NO_STREAM)
        assert lib.modegemm_path(**kw0) == 0
        out0 = torch.empty(shape, dtype=torch.cfloat, device=dev)
        lib.modegemm(torch.view_as_real(a).data_ptr(), torch.view_as_real(b).data_ptr(),
                     torch.view_as_real(out0).data_ptr(), st, **kw0)
        torch.cuda.synchronize()
        assert rel_l2(out.cpu().numpy(), ref) < TOL, name
        assert torch.equal(torch.view_as_real(out), torch.view_as_real(out0)), name


def test_backward_pair_full_size(lib):
    """sc_modegemm_pair at the metric shape (one launch of k_modegemm_dma_bwd): bit-identical to the two single
    launches and within the bar of a complex128 einsum; the same for a small batch (8 rows) at the FNO3d mode count."""
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: torch.view_as_real(t).data_ptr()
    for B, C, M in [(32, 64, 64 * 33), (8, 32, 32 * 32 * 17)]:
        torch.manual_seed(5)
        xh = torch.randn(B, C, M, dtype=torch.cfloat, device=dev)
        gh = torch.randn(B, C, M, dtype=torch.cfloat, device=dev)
        w = torch.randn(C, C, M, dtype=torch.cfloat, device=dev)
        kw_w = dict(P=C, Q=C, R=B, n_modes=M, a_sp=M, a_sr=C * M, a_sm=1, conj_a=1, b_sr=C * M, b_sq=M, b_sm=1,
                    c_sp=C * M, c_sq=M, c_sm=1)
        kw_x = dict(P=B, Q=C, R=C, n_modes=M, a_sp=C * M, a_sr=M, a_sm=1, b_sr=M, b_sq=C * M, b_sm=1, conj_b=1,
                    c_sp=C * M, c_sq=M, c_sm=1)
        assert lib.modegemm_pair_fused(kw_w, kw_x)
        gw = torch.full((C, C, M), float("nan"), dtype=torch.cfloat, device=dev)
        gx = torch.full((B, C, M), float("nan"), dtype=torch.cfloat, device=dev)
        lib.modegemm_pair(kw_w, p(xh), p(gh), p(gw), kw_x, p(gh), p(w), p(gx), st)
        gw1, gx1 = torch.empty_like(gw), torch.empty_like(gx)
        lib.modegemm(p(xh), p(gh), p(gw1), st, **kw_w)
        lib.modegemm(p(gh), p(w), p(gx1), st, **kw_x)
        torch.cuda.synchronize()
        assert torch.equal(torch.view_as_real(gw), torch.view_as_real(gw1))
        assert torch.equal(torch.view_as_real(gx), torch.view_as_real(gx1))
        x128, g128, w128 = xh.to(torch.complex128), gh.to(torch.complex128), w.to(torch.complex128)
        assert rel_l2(gw.cpu().numpy(), torch.einsum("bim,bom->iom", x128.conj(), g128).cpu().numpy()) < TOL
        assert rel_l2(gx.cpu().numpy(), torch.einsum("bom,iom->bim", g128, w128.conj()).cpu().numpy()) < TOL


@pytest.mark.parametrize("dims", [(1, 128, 128, 8256), (2, 128, 128, 8256), (3, 128, 128, 8256), (4, 128, 128, 8256),
                                  (4, 128, 64, 8322), (3, 66, 128, 4226)], ids=lambda d: "B%d_Ci%d_Co%d_M%d" % d)
def test_backward_pair_small_batch_one_pass(lib, dims):
    """k_modegemm_sb_bwd<BT,4,2> for every BT on the device: the two contractions of a small-batch
    backward pass in ONE pass over the weight (BASELINE configs[4]: hidden 128; 8 256 of its 33 024 modes = 64 mode
    tiles of 128 + a ragged one, so the complex128 reference stays small) against a complex128 einsum evaluated on the
    HOST and, bit for bit, against the two k_modegemm_sb launches it replaces (einsum_utils.py / spectral_convolution.py:21-46
    and their autograd adjoints)."""
    from neuraloperator_amd import _lib as L
    B, Ci, Co, M = dims
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: torch.view_as_real(t).data_ptr()
    torch.manual_seed(100 + B)
    xh_c = torch.randn(B, Ci, M, dtype=torch.cfloat)
    gh_c = torch.randn(B, Co, M, dtype=torch.cfloat)
    w_c = torch.randn(Ci, Co, M, dtype=torch.cfloat)
    xh, gh, w = xh_c.to(dev), gh_c.to(dev), w_c.to(dev)
    kw_w = dict(P=Ci, Q=Co, R=B, n_modes=M, a_sp=M, a_sr=Ci * M, a_sm=1, conj_a=1, b_sr=Co * M, b_sq=M, b_sm=1,
                c_sp=Co * M, c_sq=M, c_sm=1, flags=L.SC_GEMM_STREAM_C)
    kw_x = dict(P=B, Q=Ci, R=Co, n_modes=M, a_sp=Co * M, a_sr=M, a_sm=1, b_sr=M, b_sq=Co * M, b_sm=1, conj_b=1,
                c_sp=Ci * M, c_sq=M, c_sm=1)
    assert lib.modegemm_path(**kw_w) == 3 and lib.modegemm_path(**kw_x) == 3
    assert lib.modegemm_pair_path(kw_w, kw_x) == 2, "the one-pass kernel must be the one that runs"
    gw = torch.full((Ci, Co, M), float("nan"), dtype=torch.cfloat, device=dev)
    gx = torch.full((B, Ci, M), float("nan"), dtype=torch.cfloat, device=dev)
    lib.modegemm_pair(kw_w, p(xh), p(gh), p(gw), kw_x, p(gh), p(w), p(gx), st)
    gw1, gx1 = torch.empty_like(gw), torch.empty_like(gx)
    lib.modegemm(p(xh), p(gh), p(gw1), st, **kw_w)
    lib.modegemm(p(gh), p(w), p(gx1), st, **kw_x)
    torch.cuda.synchronize()
    assert torch.equal(torch.view_as_real(gw), torch.view_as_real(gw1))
    assert torch.equal(torch.view_as_real(gx), torch.view_as_real(gx1))
    # host reference on every 11th mode, the first mode tile and the ragged last one (round 5: the full complex128 einsum
    # took 35-87 s per case on the host; every element is already compared bit for bit with the two launches above)
    sel = torch.unique(torch.cat([torch.arange(0, M, 11), torch.arange(0, 128), torch.arange(M - 130, M)]))
    x128, g128, w128 = (v[..., sel].to(torch.complex128) for v in (xh_c, gh_c, w_c))
    assert rel_l2(gw.cpu()[..., sel].numpy(), torch.einsum("bim,bom->iom", x128.conj(), g128).numpy()) < TOL
    assert rel_l2(gx.cpu()[..., sel].numpy(), torch.einsum("bom,iom->bim", g128, w128.conj()).numpy()) < TOL


def test_module_dropin():
    """SpectralConv module: ctor surface, n_modes mutation (incremental FNO), grads for every
    parameter (neuralop/layers/tests/test_spectral_convolution.py:67-70, models/tests/test_fno.py)."""
    from neuraloperator_amd import SpectralConv
    from oracle import spectral_oracle as so

    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    conv = SpectralConv(3, 3, (10, 8), bias=True, implementation="factorized", factorization=None,
                        rank=0.5, fixed_rank_modes=False, separable=False, complex_data=False,
                        fno_block_precision="full", decomposition_kwargs=dict(),
                        resolution_scaling_factor=None, max_n_modes=None,
                        enforce_hermitian_symmetry=True).to(dev)
    x = torch.randn(2, 3, 12, 12, device=dev, requires_grad=True)
    y = conv(x)
    assert y.shape == (2, 3, 12, 12) and y.dtype == torch.float32
    assert conv.transform(x) is x
    y.sum().backward()
    for p in conv.parameters():
        assert p.grad is not None
    yo = so.forward_torch(x.detach().cpu(), conv.weight.tensor.detach().cpu(), conv.bias.detach().cpu(),
                          conv.n_modes, conv.max_n_modes)
    assert rel_l2(y.detach().cpu().numpy(), yo.numpy()) < TOL
    conv.n_modes = (6, 6)
    assert conv.n_modes == [6, 4]
    y2 = conv(x)
    yo2 = so.forward_torch(x.detach().cpu(), conv.weight.tensor.detach().cpu(), conv.bias.detach().cpu(),
                           conv.n_modes, conv.max_n_modes)
    assert rel_l2(y2.detach().cpu().numpy(), yo2.numpy()) < TOL
    with pytest.raises(RuntimeError):
        conv(torch.randn(2, 3, 12, 12))        # CPU tensor: loud failure, no fallback


def test_module_edge_inputs():
    """Empty batch, non-contiguous input, fp64 / bf16 inputs (computed in fp32 like the reference's
    fp32 spectral path), odd n_modes, grid smaller than the modes."""
    from neuraloperator_amd import SpectralConv
    from oracle import spectral_oracle as so

    dev = torch.device("cuda:0")
    torch.manual_seed(9)
    conv = SpectralConv(4, 6, (7, 9)).to(dev)
    w, b = conv.weight.tensor.detach().cpu(), conv.bias.detach().cpu()
    # empty batch
    y0 = conv(torch.randn(0, 4, 16, 20, device=dev))
    assert tuple(y0.shape) == (0, 6, 16, 20)
    # non-contiguous view of a larger tensor
    big = torch.randn(3, 4, 16, 40, device=dev)
    xv = big[:, :, :, ::2]
    assert not xv.is_contiguous()
    y = conv(xv)
    yo = so.forward_torch(xv.cpu().contiguous(), w, b, conv.n_modes, conv.max_n_modes)
    assert rel_l2(y.detach().cpu().numpy(), yo.numpy()) < TOL
    # grid smaller than the modes along one dim (6 rows < 7 modes)
    xs = torch.randn(2, 4, 6, 20, device=dev)
    ys = conv(xs)
    yso = so.forward_torch(xs.cpu(), w, b, conv.n_modes, conv.max_n_modes)
    assert rel_l2(ys.detach().cpu().numpy(), yso.numpy()) < TOL
    # double input: engine computes in fp32 and returns fp32
    xd = torch.randn(2, 4, 16, 20, device=dev, dtype=torch.float64)
    yd = conv(xd)
    assert yd.dtype == torch.float32
    ydo = so.forward_torch(xd.float().cpu(), w, b, conv.n_modes, conv.max_n_modes)
    assert rel_l2(yd.detach().cpu().numpy(), ydo.numpy()) < TOL
    # wrong rank / channel count fail loudly
    with pytest.raises(ValueError):
        conv(torch.randn(2, 4, 16, device=dev))
    with pytest.raises(ValueError):
        conv(torch.randn(2, 5, 16, 20, device=dev))


@pytest.mark.parametrize("name", [n for n in FACT_GOLDEN if n.startswith("tucker")])
def test_tucker_factorized_native_matches_golden(name):
    """implementation="factorized" + Tucker weight: the contraction runs on the pairwise
    sc_modegemm chain (never forms the dense weight); outputs and the gradients of the core and of
    every factor against the verbatim reference's _contract_tucker (golden vectors)."""
    from neuraloperator_amd import SpectralConv
    g = load_golden(name)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(g["x"]).to(dev).requires_grad_(True)
    nd = x.ndim - 2
    ci, co = g["factor_0"].shape[0], g["factor_1"].shape[0]
    conv = SpectralConv(ci, co, tuple(int(v) for v in g["ctor_n_modes"]), factorization="Tucker",
                        implementation="factorized", rank=float(g["rank"])).to(dev)
    assert tuple(conv.weight.core.shape) == tuple(g["core"].shape)
    with torch.no_grad():
        conv.weight.core.copy_(torch.from_numpy(g["core"]))
        for i in range(nd + 2):
            conv.weight.factors[i].copy_(torch.from_numpy(g[f"factor_{i}"]))
        conv.bias.copy_(torch.from_numpy(g["bias"]))
    conv.n_modes = tuple(int(v) for v in g["n_modes_attr"][:-1]) + (2 * (int(g["n_modes_attr"][-1]) - 1),)
    assert list(conv.n_modes) == list(g["n_modes_attr"])
    y = conv(x)
    y.backward(torch.from_numpy(g["g"]).to(dev))
    assert rel_l2(y.detach().cpu().numpy(), g["y"]) < TOL
    assert rel_l2(x.grad.cpu().numpy(), g["gx"]) < TOL
    assert rel_l2(conv.bias.grad.cpu().numpy(), g["gbias"]) < TOL
    assert rel_l2(conv.weight.core.grad.cpu().numpy(), g["g_core"]) < TOL
    for i in range(nd + 2):
        assert rel_l2(conv.weight.factors[i].grad.cpu().numpy(), g[f"g_factor_{i}"]) < TOL, i


@pytest.mark.parametrize("impl", ["factorized", "reconstructed"])
@pytest.mark.parametrize("name", [n for n in FACT_GOLDEN if n.startswith("cp")])
def test_cp_native_matches_golden(name, impl):
    """CP weight on the sc_modegemm chain (factorized: never forms the dense weight; reconstructed: one
    launch builds it) against the verbatim reference's _contract_cp, gradients of weights and factors."""
    from neuraloperator_amd import SpectralConv
    g = load_golden(name)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(g["x"]).to(dev).requires_grad_(True)
    nd = x.ndim - 2
    ci, co = g["factor_0"].shape[0], g["factor_1"].shape[0]
    conv = SpectralConv(ci, co, tuple(int(v) for v in g["ctor_n_modes"]), factorization="CP",
                        implementation=impl, rank=int(g["weights"].shape[0])).to(dev)
    with torch.no_grad():
        conv.weight.weights.copy_(torch.from_numpy(g["weights"]))
        for i in range(nd + 2):
            conv.weight.factors[i].copy_(torch.from_numpy(g[f"factor_{i}"]))
        conv.bias.copy_(torch.from_numpy(g["bias"]))
    y = conv(x)
    y.backward(torch.from_numpy(g["g"]).to(dev))
    assert rel_l2(y.detach().cpu().numpy(), g["y"]) < TOL
    assert rel_l2(x.grad.cpu().numpy(), g["gx"]) < TOL
    assert rel_l2(conv.bias.grad.cpu().numpy(), g["gbias"]) < TOL
    assert rel_l2(conv.weight.weights.grad.cpu().numpy(), g["g_weights"]) < TOL
    for i in range(nd + 2):
        assert rel_l2(conv.weight.factors[i].grad.cpu().numpy(), g[f"g_factor_{i}"]) < TOL, i


@pytest.mark.parametrize("fac", ["Tucker", "CP", "TT"])
def test_module_factorized_matches_dense(fac):
    """factorized weight == dense conv with weight.to_tensor()
    (the reference's identity, test_spectral_convolution.py:54-65)."""
    from neuraloperator_amd import SpectralConv
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    conv = SpectralConv(3, 3, (10, 8), bias=False, factorization=fac, implementation="factorized").to(dev)
    dense = SpectralConv(3, 3, (10, 8), bias=False).to(dev)
    with torch.no_grad():
        dense.weight.tensor.copy_(conv.weight.to_tensor())
    x = torch.randn(2, 3, 12, 12, device=dev, requires_grad=True)
    y = conv(x)
    yd = dense(x)
    assert rel_l2(y.detach().cpu().numpy(), yd.detach().cpu().numpy()) < TOL
    y.sum().backward()
    for p in conv.parameters():
        assert p.grad is not None and torch.isfinite(torch.view_as_real(p.grad)).all()


# ------------------------------------------------------------------------------------------
# constructor variants of the drop-in module against golden vectors of the verbatim reference:
# separable, TT, resolution_scaling_factor / output_shape, complex_data, skip-path transform
# ------------------------------------------------------------------------------------------
VARIANT_GOLDEN = [n for n in golden_names() if n.startswith(("sep_", "tt_", "res_", "cplx_"))]


@pytest.mark.parametrize("name", VARIANT_GOLDEN)
def test_module_variants_match_golden(name):
    import json
    from neuraloperator_amd import SpectralConv
    g = load_golden(name)
    kw = json.loads(str(g["ctor_kwargs"]))
    dev = torch.device("cuda:0")
    x = torch.from_numpy(g["x"]).to(dev).requires_grad_(True)
    ci, co = x.shape[1], g["y"].shape[1]
    n_par = sum(1 for k in g if k.startswith("param_name_"))
    if str(g["weight_kind"]) == "TTTensor":
        # the rank RULE is tensorly's and unpinned by any reference test: take the bond ranks
        # of the fixture's cores so that the contraction itself is what gets compared
        kw["rank"] = [int(g[f"param_{i}"].shape[0]) for i in range(n_par)] + [1]
    conv = SpectralConv(ci, co, tuple(int(v) for v in g["ctor_n_modes"]), **kw).to(dev)
    assert list(conv.n_modes) == [int(v) for v in g["n_modes_attr"]]
    # the fixtures name factor parameters after the stub's nn.ParameterList ("factors.0"); the module registers them
    # under tltorch's FactorList names ("factors.factor_0")
    params = {k.replace("factors.factor_", "factors."): v for k, v in conv.weight.named_parameters()}
    assert len(params) == n_par
    with torch.no_grad():
        for i in range(n_par):
            p = params[str(g[f"param_name_{i}"])]
            assert tuple(p.shape) == tuple(g[f"param_{i}"].shape), (i, p.shape)
            p.copy_(torch.from_numpy(g[f"param_{i}"]))
        conv.bias.copy_(torch.from_numpy(g["bias"]))
    out_shape = tuple(int(v) for v in g["output_shape"]) or None
    y = conv(x, output_shape=out_shape) if out_shape else conv(x)
    assert tuple(y.shape) == tuple(g["y"].shape) and y.dtype == torch.from_numpy(g["y"]).dtype
    y.backward(torch.from_numpy(g["g"]).to(dev))
    assert rel_l2(y.detach().cpu().numpy(), g["y"]) < TOL
    assert rel_l2(x.grad.cpu().numpy(), g["gx"]) < TOL
    assert rel_l2(conv.bias.grad.cpu().numpy(), g["gbias"]) < TOL
    for i in range(n_par):
        p = params[str(g[f"param_name_{i}"])]
        assert rel_l2(p.grad.cpu().numpy(), g[f"g_param_{i}"]) < TOL, str(g[f"param_name_{i}"])


@pytest.mark.parametrize("name", golden_names("xform_"))
def test_module_transform_matches_golden(name):
    """SpectralConv.transform (the skip path of a resolution-changing FNO block, fno_block.py:380-384)"""
    from neuraloperator_amd import SpectralConv
    g = load_golden(name)
    dev = torch.device("cuda:0")
    x = torch.from_numpy(g["x"]).to(dev)
    conv = SpectralConv(2, 2, tuple(4 for _ in x.shape[2:])).to(dev)
    t = conv.transform(x, output_shape=tuple(int(v) for v in g["output_shape"]))
    assert rel_l2(t.cpu().numpy(), g["t"]) < TOL
    assert conv.transform(x) is x                                   # identity without a resolution change


@pytest.mark.parametrize("fac,impl", [("Tucker", "factorized"), ("Tucker", "reconstructed"), ("TT", "factorized"),
                                      ("CP", "factorized")])
def test_factorized_chain_at_matrix_core_sizes(fac, impl):
    """64 channels, batch 32: the pairwise steps with ragged ranks (Tucker 0.3 -> ~40) run on the matrix-core
    contraction.  Reference: the dense module with weight.to_tensor(), and torch autograd through to_tensor()
    for the factor gradients (the identity test_spectral_convolution.py:54-65 pins)."""
    from neuraloperator_amd import SpectralConv
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    kw = dict(rank=0.3) if fac != "CP" else dict(rank=48)
    conv = SpectralConv(64, 64, (16, 16), factorization=fac, implementation=impl, **kw).to(dev)
    with torch.no_grad():
        for p in conv.weight.parameters():
            p.copy_(torch.randn_like(p) * 0.4)
    dense = SpectralConv(64, 64, (16, 16)).to(dev)
    with torch.no_grad():
        dense.weight.tensor.copy_(conv.weight.to_tensor())
        dense.bias.copy_(conv.bias)
    x = torch.randn(32, 64, 32, 32, device=dev, requires_grad=True)
    xd = x.detach().clone().requires_grad_(True)
    g = torch.randn(32, 64, 32, 32, device=dev)
    y, yd = conv(x), dense(xd)
    y.backward(g)
    yd.backward(g)
    assert rel_l2(y.detach().cpu().numpy(), yd.detach().cpu().numpy()) < TOL
    assert rel_l2(x.grad.cpu().numpy(), xd.grad.cpu().numpy()) < TOL
    # factor gradients: push the dense weight gradient through to_tensor() with torch autograd (host glue)
    ref = SpectralConv(64, 64, (16, 16), factorization=fac, implementation=impl, **kw).to(dev)
    ref.load_state_dict(conv.state_dict())
    ref.weight.to_tensor().backward(dense.weight.tensor.grad)
    for (n1, p1), (n2, p2) in zip(conv.weight.named_parameters(), ref.weight.named_parameters()):
        assert rel_l2(p1.grad.cpu().numpy(), p2.grad.cpu().numpy()) < 2 * TOL, n1


@pytest.mark.parametrize("name", ["half_2d", "mixed_2d", "mixed_3d"])
def test_block_precision_half_mixed(name):
    """fno_block_precision half / mixed (spectral_convolution.py:436-459): values rounded to float16 at the
    reference's cast points, the contraction with the arithmetic of einsum_complexhalf (SC_GEMM_F16), fp32
    transforms; golden vectors from the oracle's restatement, whose contraction is pinned bit for bit against the
    verbatim einsum_utils on the CPU.  Output dtype as upstream: fp32 with a bias (half + fp32 parameter promotes),
    fp16 without."""
    from neuraloperator_amd import SpectralConv
    dev = torch.device("cuda:0")
    g = load_golden(name)
    prec = str(g["precision"])
    ci, co = g["w"].shape[:2]
    nm = tuple(int(v) for v in g["ctor_n_modes"])
    conv = SpectralConv(ci, co, nm, fno_block_precision=prec).to(dev)
    with torch.no_grad():
        conv.weight.tensor.copy_(torch.from_numpy(g["w"]))
        conv.bias.copy_(torch.from_numpy(g["bias"]))
    x = torch.from_numpy(g["x"]).to(dev).requires_grad_(True)
    y = conv(x)
    assert y.dtype == torch.float32
    y.backward(torch.from_numpy(g["g"]).to(dev))
    bias = torch.from_numpy(g["bias"])
    yb, rb = y.detach().cpu() - bias, torch.from_numpy(g["y"]) - bias
    step = torch.maximum(rb.abs(), torch.tensor(6.1e-5)) * 2.0 ** -10             # one float16 step of the value
    assert bool(((yb - rb).abs() <= 1.01 * step).all())
    assert ((yb - rb).abs() <= 1e-7).float().mean().item() > 0.98
    assert rel_l2(x.grad.cpu().numpy(), g["gx"]) < 2e-3                            # float16 gradient arithmetic
    assert rel_l2(conv.weight.tensor.grad.cpu().numpy(), g["gw"]) < 2e-3
    assert rel_l2(conv.bias.grad.cpu().numpy(), g["gbias"]) < 1e-5
    nb = SpectralConv(ci, co, nm, fno_block_precision=prec, bias=False).to(dev)
    assert nb(x.detach()).dtype == torch.float16
    with pytest.raises(ValueError):
        SpectralConv(4, 4, (8, 8), fno_block_precision="quarter")


@pytest.mark.parametrize("run_modes,out_shape,separable,cplx", [((10, 8), None, False, False), (None, (40, 30), False, False),
                                                                ((9, 12), (24, 20), False, False), ((10, 8), None, True, False),
                                                                (None, None, False, True), ((10, 8), None, False, True)],
                         ids=["fewer_modes", "finer_grid", "fewer_modes_coarser_grid", "separable_fewer_modes",
                              "complex_data", "complex_data_fewer_modes"])
def test_mode_parallel_general_path_on_device(run_modes, out_shape, separable, cplx):
    """Runtime-reduced n_modes / a different output grid on the mode-parallel layer (round 3, session 2:
    ModeParallelSpectralConv._forward_general on engine.EngineOps, one rank, no process group: the exchanges
    degenerate; their sharding logic is covered by the world-size-2 gloo tests) against the CPU oracle."""
    from neuraloperator_amd.mpu import ModeParallelSpectralConv
    from oracle import spectral_oracle as so
    dev = torch.device("cuda:0")
    torch.manual_seed(4)
    ci = co = 6 if separable else 6
    co = ci if separable else 5
    conv = ModeParallelSpectralConv(ci, co, (16, 12), separable=separable, complex_data=cplx).to(dev)
    if run_modes is not None:
        conv.n_modes = run_modes
    x = torch.randn(3, ci, 32, 24, dtype=torch.cfloat if cplx else torch.float32)
    xd = x.to(dev).requires_grad_(True)
    y = conv(xd, output_shape=out_shape)
    g = torch.randn(*y.shape, dtype=y.dtype)
    y.backward(g.to(dev))
    torch.cuda.synchronize()
    xc = x.clone().requires_grad_(True)
    wc = conv.weight.detach().cpu().clone().requires_grad_(True)
    bc = conv.bias.detach().cpu().clone().requires_grad_(True)
    yo = so.forward_torch(xc, wc, bc, conv.n_modes, conv.max_n_modes, separable=separable, output_shape=out_shape,
                          complex_data=cplx)
    yo.backward(g)
    assert rel_l2(y.detach().cpu().numpy(), yo.detach().numpy()) < TOL
    assert rel_l2(xd.grad.cpu().numpy(), xc.grad.numpy()) < TOL
    assert rel_l2(conv.weight.grad.cpu().numpy(), wc.grad.numpy()) < TOL
    assert rel_l2(conv.bias.grad.cpu().numpy(), bc.grad.numpy()) < TOL
    if out_shape is not None and not cplx:
        assert list(conv.transform(xd.detach(), output_shape=out_shape).shape[2:]) == list(out_shape)


def test_mode_parallel_layer_on_device_single_rank():
    """The mode-parallel layer with the engine's stage ops on the GPU (RCCL group of one rank: the all-to-alls
    degenerate, everything else -- stage plumbing, autograd through both transforms and the contraction --
    is the multi-GPU code path; the sharding itself is covered by the world-size-2 / 8 gloo tests).  Reference =
    the CPU oracle (forward_torch + autograd, Tucker: the oracle's pairwise contraction), not the plain engine layer."""
    import os
    import socket
    import torch.distributed as dist
    from neuraloperator_amd import SpectralConv
    from neuraloperator_amd.mpu import ModeParallelSpectralConv, comm
    port = comm.free_port()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    dev = torch.device("cuda:0")
    comm.init(model_parallel_size=1, backend="nccl")
    try:
        torch.manual_seed(2)
        ref = SpectralConv(6, 5, (16, 12)).to(dev)
        mp_conv = ModeParallelSpectralConv(6, 5, (16, 12)).to(dev)
        with torch.no_grad():
            mp_conv.weight.copy_(ref.weight.tensor)
            mp_conv.bias.copy_(ref.bias)
        x = torch.randn(4, 6, 32, 24, device=dev, requires_grad=True)
        g = torch.randn(4, 5, 32, 24, device=dev)
        y = mp_conv(x)
        y.backward(g)
        mp_conv.reduce_replicated_grads()
        yo, gxo, gwo, gbo = _oracle_layer(x, ref.weight.tensor, ref.bias, g, ref.n_modes)
        assert rel_l2(y.detach().cpu().numpy(), yo) < TOL
        assert rel_l2(x.grad.cpu().numpy(), gxo) < TOL
        assert rel_l2(mp_conv.weight.grad.cpu().numpy(), gwo) < TOL
        assert rel_l2(mp_conv.bias.grad.cpu().numpy(), gbo) < TOL
        # one sample per rank, channel chunks (round 4): the list form of the RCCL all-to-all moves slabs of the
        # contraction's operand / result in place (ragged chunks: 6 -> 2 + 2 + 2 input, 5 -> 1 + 2 + 2 output channels)
        cc = ModeParallelSpectralConv(6, 5, (16, 12), comm_chunks=3, chunk_dim="channels").to(dev)
        with torch.no_grad():
            cc.weight.copy_(ref.weight.tensor)
            cc.bias.copy_(ref.bias)
        x1 = x.detach()[:1].clone().requires_grad_(True)
        y1 = cc(x1)
        y1.backward(g[:1])
        yo1, gxo1, gwo1, gbo1 = _oracle_layer(x1, ref.weight.tensor, ref.bias, g[:1], ref.n_modes)
        assert rel_l2(y1.detach().cpu().numpy(), yo1) < TOL
        assert rel_l2(x1.grad.cpu().numpy(), gxo1) < TOL
        assert rel_l2(cc.weight.grad.cpu().numpy(), gwo1) < TOL
        assert rel_l2(cc.bias.grad.cpu().numpy(), gbo1) < TOL
        # TFNO weights in the same layer: replicated core / factors, the first mode dim's factor sharded (here: whole)
        from oracle import spectral_oracle as so
        tref = SpectralConv(6, 5, (16, 12), factorization="tucker", rank=0.5, implementation="factorized")
        tmp = ModeParallelSpectralConv(6, 5, (16, 12), factorization="tucker", rank=0.5).to(dev)
        assert tuple(tmp.core.shape) == tuple(tref.weight.core.shape)
        with torch.no_grad():
            for q in list(tref.weight.parameters()):
                q.mul_(8.0)                                        # O(1) outputs
            tmp.core.copy_(tref.weight.core)
            for f, fr in zip(tmp.factors, tref.weight.factors):
                f.copy_(fr)
            tmp.bias.copy_(tref.bias)
        x2 = x.detach().clone().requires_grad_(True)
        y2 = tmp(x2)
        y2.backward(g)
        tmp.reduce_replicated_grads()
        core = tref.weight.core.detach().clone().requires_grad_(True)
        facs = [f.detach().clone().requires_grad_(True) for f in tref.weight.factors]
        y3, gx3, _, gb3 = _oracle_layer(x, so.reconstruct_tucker(core, facs).detach(), tref.bias, g, tref.n_modes,
                                        contract=lambda xk, wk: so.contract_tucker(xk, core, facs))
        assert rel_l2(y2.detach().cpu().numpy(), y3) < TOL
        assert rel_l2(x2.grad.cpu().numpy(), gx3) < TOL
        assert rel_l2(tmp.bias.grad.cpu().numpy(), gb3) < TOL
        assert rel_l2(tmp.core.grad.cpu().numpy(), core.grad.numpy()) < TOL
        for f, fr in zip(tmp.factors, facs):
            assert rel_l2(f.grad.cpu().numpy(), fr.grad.numpy()) < TOL
    finally:
        comm.cleanup()
        if dist.is_initialized():
            dist.destroy_process_group()
        for k in ("MASTER_ADDR", "MASTER_PORT", "RANK", "WORLD_SIZE", "LOCAL_RANK"):
            os.environ.pop(k, None)


@pytest.mark.parametrize("kind", ["cp", "tt", "separable"])
def test_mode_parallel_variants_on_device_single_rank(kind):
    """CP / TT / separable weights of the mode-parallel layer (round 3) through the engine's raw ops on the GPU (one rank,
    no process group: the dense block rebuilt on the engine with autograd, the separable contraction as an engine
    launch) against the CPU oracle with the reconstructed weight."""
    from oracle import spectral_oracle as so
    from neuraloperator_amd.mpu import ModeParallelSpectralConv
    dev = torch.device("cuda:0")
    torch.manual_seed(8)
    ci, co, modes, spatial = 6, (6 if kind == "separable" else 5), (16, 12), (32, 24)
    kw = dict(separable=True) if kind == "separable" else dict(factorization=kind, rank=0.5)
    conv = ModeParallelSpectralConv(ci, co, modes, **kw).to(dev)
    with torch.no_grad():
        for q in conv.parameters():
            if q.is_complex():
                q.copy_(torch.randn(q.shape, dtype=torch.cfloat) * 0.6)
    x = torch.randn(3, ci, *spatial, device=dev, requires_grad=True)
    g = torch.randn(3, co, *spatial, device=dev)
    y = conv(x)
    y.backward(g)
    leaves = [q.detach().cpu().clone().requires_grad_(True) for q in conv.parameters() if q.is_complex()]
    names = [n for n, q in conv.named_parameters() if q.is_complex()]
    if kind == "separable":
        w = leaves[0]
    elif kind == "cp":
        w = so.reconstruct_cp(leaves[names.index("cp_weights")], [leaves[names.index(f"factors.factor_{i}")] for i in range(4)])
    else:
        w = so.reconstruct_tt([leaves[names.index(f"factors.factor_{i}")] for i in range(4)])
    xc = x.detach().cpu().requires_grad_(True)
    bc = conv.bias.detach().cpu().requires_grad_(True)
    nm = list(conv.n_modes)
    yo = so.forward_torch(xc, w, bc, nm, nm, separable=(kind == "separable"),
                          contract=so.contract_dense_separable if kind == "separable" else so.contract_dense)
    yo.backward(g.cpu())
    assert rel_l2(y.detach().cpu().numpy(), yo.detach().numpy()) < TOL
    assert rel_l2(x.grad.cpu().numpy(), xc.grad.numpy()) < TOL
    assert rel_l2(conv.bias.grad.cpu().numpy(), bc.grad.numpy()) < TOL
    grads = {n: q.grad for n, q in conv.named_parameters() if q.is_complex()}
    for n, lf in zip(names, leaves):
        assert rel_l2(grads[n].cpu().numpy(), lf.grad.numpy()) < 2e-5, n


@pytest.mark.parametrize("spatial,modes,P", [((64, 256), (16, 12), 4), ((256, 256), (64, 64), 8), ((128, 256), (10, 64), 4),
                                             ((24, 20), (8, 10), 2), ((16, 128, 128), (8, 32, 32), 8),
                                             ((12, 16, 20), (5, 8, 8), 3),
                                             # round 5: k_ax128 / k_ax64 address the shards natively
                                             ((128, 128, 128), (32, 32, 32), 8), ((128, 128, 128), (20, 32, 32), 7),
                                             ((64, 64, 64), (16, 16, 16), 4),
                                             # ... and fewer kept rows than blocks can fill: the last block(s) EMPTY
                                             ((128, 128, 128), (20, 32, 32), 8), ((64, 256), (6, 12), 4), ((24, 20), (5, 10), 4)])
def test_sharded_transforms_on_device(spatial, modes, P):
    """The engine's sharded-spectrum stages (round 3: the transforms of a mode-parallel layer write / read the
    rank-major all-to-all buffer [P][n][c][rows][rest] in place) on the GPU: bit-identical to the plain stage plus the
    permutation it replaces -- fused 2-D kernels (native addressing), plane / size-agnostic routes (one permutation
    launch inside the call), padded rows -- and the four of them compose to the CPU oracle's layer."""
    from neuraloperator_amd.engine import EngineRawOps
    from neuraloperator_amd.modes import halve_last_mode, kept_block
    dev = torch.device("cuda:0")
    torch.manual_seed(12)
    nm = halve_last_mode(modes)
    kept, _ = kept_block(list(spatial), nm, nm)
    k1 = kept[0]
    rows = -(-k1 // P)
    n, ci, co = 2, 3, 4
    ops = EngineRawOps()
    x = torch.randn(n, ci, *spatial, device=dev)
    g = torch.randn(n, co, *spatial, device=dev)
    bias = torch.randn(co, device=dev)

    def to_shards(xh):                                   # (n, c, k1, rest..) complex -> [P, n, c, rows, rest.., 2]
        xr = torch.view_as_real(xh)
        pad = xr.new_zeros((xr.shape[0], xr.shape[1], P * rows, *xr.shape[3:]))
        pad[:, :, :k1] = xr
        return pad.unflatten(2, (P, rows)).movedim(2, 0).contiguous()

    xh = ops.fwd(x, kept)
    buf = ops.fwd_sharded(x, kept, P, rows)
    assert torch.equal(buf, to_shards(xh))
    gh, gb = ops.inv_adjoint(g, kept, want_bias=True)
    gbuf, gb2 = ops.inv_adjoint_sharded(g, kept, P, rows, want_bias=True)
    assert torch.equal(gbuf, to_shards(gh)) and torch.equal(gb, gb2)
    yh = torch.randn(n, co, *kept, dtype=torch.cfloat, device=dev)
    y0 = ops.inv(yh, bias, list(spatial))
    y1 = ops.inv_sharded(to_shards(yh), bias, list(spatial), k1)
    assert torch.equal(y0, y1)
    gx0 = ops.fwd_adjoint(yh[:, :ci], list(spatial))
    gx1 = ops.fwd_adjoint_sharded(to_shards(yh[:, :ci].contiguous()), list(spatial), k1)
    assert torch.equal(gx0, gx1)
    # and against the oracle: sharded forward -> (undo the sharding on the host) -> contraction -> sharded inverse
    w = torch.randn(ci, co, *kept, dtype=torch.cfloat, device=dev) * 0.3
    xh_from_buf = torch.view_as_complex(buf.movedim(0, 2).flatten(2, 3)[:, :, :k1].contiguous())
    y = ops.inv_sharded(to_shards(ops.contract(xh_from_buf, w)), bias, list(spatial), k1)
    yo, _, _, _ = _oracle_layer(x, w, bias.reshape(co, *(1,) * len(spatial)), g, nm)
    assert rel_l2(y.cpu().numpy(), yo) < TOL


@pytest.mark.parametrize("spatial,modes", [((32, 24), (16, 12)), ((12, 16, 20), (6, 8, 8)), ((64, 256), (16, 16))])
def test_spatial_parallel_layer_on_device_single_rank(spatial, modes):
    """The spatially decomposed layer with the engine's stage ops on the GPU, one rank (no process
    group: the all-to-alls degenerate): the (N-1)-d real plans with the rows folded into the channel count, the 1-d
    complex axis plans with the centred frequency map, the contraction and autograd through all of them against
    the CPU oracle (forward_torch + autograd).  Row sharding / padding / exchange: world-size-2 gloo test."""
    from neuraloperator_amd import SpectralConv
    from neuraloperator_amd.mpu import SpatialParallelSpectralConv

    dev = torch.device("cuda:0")
    torch.manual_seed(4)
    ref = SpectralConv(6, 5, modes).to(dev)
    sp = SpatialParallelSpectralConv(6, 5, modes).to(dev)
    assert sp.P == 1
    with torch.no_grad():
        sp.weight.copy_(ref.weight.tensor)
        sp.bias.copy_(ref.bias)
    x = torch.randn(3, 6, *spatial, device=dev, requires_grad=True)
    g = torch.randn(3, 5, *spatial, device=dev)
    y = sp(x)
    y.backward(g)
    yo, gxo, gwo, gbo = _oracle_layer(x, ref.weight.tensor, ref.bias, g, ref.n_modes)     # the CPU oracle, not the engine
    assert rel_l2(y.detach().cpu().numpy(), yo) < TOL
    assert rel_l2(x.grad.cpu().numpy(), gxo) < TOL
    assert rel_l2(sp.weight.grad.cpu().numpy(), gwo) < TOL
    assert rel_l2(sp.bias.grad.cpu().numpy(), gbo) < TOL


@pytest.mark.parametrize("spatial,modes,fac,out_shape", [((32, 24), (16, 12), "tucker", None), ((32, 24), (16, 12), "cp", None),
                                                          ((12, 16, 20), (6, 8, 8), "tt", None),
                                                          ((32, 24), (16, 12), "dense", (48, 40)),
                                                          ((32, 24), (16, 12), "tucker", (24, 20)),
                                                          ((64, 256), (16, 16), "dense", (128, 256))])
def test_spatial_parallel_variants_on_device_single_rank(spatial, modes, fac, out_shape):
    """Round 5: the spatially decomposed layer with factorized weights (the rank's mode columns reconstructed from the
    replicated factors, contracted on the engine) and with a change of resolution (the first-dim inverse pass runs to
    the output grid with the reference's non-centred row map, the last-dims pass to the output columns), engine stage
    ops, one rank, against the CPU oracle with the reconstructed dense weight."""
    from oracle import spectral_oracle as so
    from neuraloperator_amd.modes import halve_last_mode
    from neuraloperator_amd.mpu import SpatialParallelSpectralConv

    dev = torch.device("cuda:0")
    torch.manual_seed(14)
    nm = halve_last_mode(modes)
    sp = SpatialParallelSpectralConv(4, 3, modes, factorization=fac, rank=0.5).to(dev)
    x = torch.randn(2, 4, *spatial, device=dev, requires_grad=True)
    og = list(out_shape) if out_shape is not None else list(spatial)
    g = torch.randn(2, 3, *og, device=dev)
    y = sp(x, output_shape=out_shape)
    assert list(y.shape) == [2, 3, *og]
    y.backward(g)
    w = (sp.weight if fac == "dense" else sp.weight.to_tensor()).detach().cpu()
    xc = x.detach().cpu().requires_grad_(True)
    bc = sp.bias.detach().cpu().requires_grad_(True)
    if fac == "dense":
        wc = w.clone().requires_grad_(True)
    else:
        from neuraloperator_amd.factorized import SpectralWeight
        ref = SpectralWeight.new((4, 3, *nm), rank=0.5, factorization=fac)
        with torch.no_grad():
            for q, r in zip(ref.parameters(), sp.weight.parameters()):
                q.copy_(r.cpu())
        wc = ref.to_tensor()
    yo = so.forward_torch(xc, wc, bc, nm, nm, output_shape=out_shape)
    yo.backward(g.cpu())
    assert rel_l2(y.detach().cpu().numpy(), yo.detach().numpy()) < TOL
    assert rel_l2(x.grad.cpu().numpy(), xc.grad.numpy()) < TOL
    assert rel_l2(sp.bias.grad.cpu().numpy(), bc.grad.numpy()) < TOL
    if fac == "dense":
        assert rel_l2(sp.weight.grad.cpu().numpy(), wc.grad.numpy()) < TOL
    else:
        for q, r in zip(sp.weight.parameters(), ref.parameters()):
            assert rel_l2(torch.view_as_real(q.grad).cpu().numpy(), torch.view_as_real(r.grad).numpy()) < TOL


@pytest.mark.parametrize("cfg", [
    dict(spatial=(32, 24), modes=(16, 12), run_modes=(12, 8)),                       # runtime n_modes
    dict(spatial=(12, 16, 20), modes=(6, 8, 8), run_modes=(5, 6, 6)),                # 3-d: the column dim is a centred one
    dict(spatial=(12, 16, 20), modes=(6, 8, 8), run_modes=(4, 4, 6), fac="tucker"),
    dict(spatial=(8, 24), modes=(16, 12)),                                           # the grid is smaller than the modes
    dict(spatial=(32, 24), modes=(16, 12), complex=True),
    dict(spatial=(12, 16, 10), modes=(6, 8, 5), complex=True, run_modes=(4, 6, 3)),
    dict(spatial=(32, 24), modes=(16, 12), complex=True, out_shape=(48, 20)),
    dict(spatial=(12, 16, 20), modes=(6, 8, 8), out_shape=(12, 24, 20)),             # the middle dim changes
    dict(spatial=(12, 16, 20), modes=(8, 12, 8), out_shape=(16, 10, 28)),            # every dim, the middle one coarser than its modes
    dict(spatial=(32, 24), modes=(16, 12), separable=True, run_modes=(12, 8)),
], ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()).replace(" ", ""))
def test_spatial_parallel_round6_variants_on_device_single_rank(cfg):
    """Round 6: the spatially decomposed layer with runtime n_modes (the used centred sub-block of the stored weight, the
    used columns at their place of the padded column layout), a grid smaller than the modes, complex_data (complex
    local plans + the reference's last-dim rule) and a change of resolution along every dim (synthesis maps on the local
    plan and on the axis plan) -- engine stage ops, one rank, against the CPU oracle.  Sharding: world-2 gloo test."""
    from oracle import spectral_oracle as so
    from neuraloperator_amd.modes import halve_last_mode
    from neuraloperator_amd.mpu import SpatialParallelSpectralConv

    dev = torch.device("cuda:0")
    torch.manual_seed(24)
    spatial, modes, cplx, fac = cfg["spatial"], cfg["modes"], cfg.get("complex", False), cfg.get("fac", "dense")
    out_shape, sep = cfg.get("out_shape"), cfg.get("separable", False)
    mx = halve_last_mode(modes, cplx)
    co = 4 if sep else 3
    sp = SpatialParallelSpectralConv(4, co, modes, factorization=fac, rank=0.5, complex_data=cplx, separable=sep).to(dev)
    if cfg.get("run_modes") is not None:
        sp.n_modes = cfg["run_modes"]
    nm = list(sp.n_modes)
    dt = torch.cfloat if cplx else torch.float32
    x = torch.randn(2, 4, *spatial, device=dev, dtype=dt, requires_grad=True)
    og = list(out_shape) if out_shape is not None else list(spatial)
    g = torch.randn(2, co, *og, device=dev, dtype=dt)
    y = sp(x, output_shape=out_shape)
    assert list(y.shape) == [2, co, *og]
    y.backward(g)
    xc = x.detach().cpu().requires_grad_(True)
    bc = sp.bias.detach().cpu().requires_grad_(True)
    if fac == "dense":
        wc = sp.weight.detach().cpu().clone().requires_grad_(True)
    else:
        from neuraloperator_amd.factorized import SpectralWeight
        ref = SpectralWeight.new(((4,) if sep else (4, 3)) + tuple(mx), rank=0.5, factorization=fac)
        with torch.no_grad():
            for q, r in zip(ref.parameters(), sp.weight.parameters()):
                q.copy_(r.cpu())
        wc = ref.to_tensor()
    yo = so.forward_torch(xc, wc, bc, nm, mx, output_shape=out_shape, complex_data=cplx, separable=sep)
    yo.backward(g.cpu())
    num = lambda t: torch.view_as_real(t.detach().cpu().contiguous()).numpy() if t.is_complex() else t.detach().cpu().numpy()
    assert rel_l2(num(y), num(yo)) < TOL
    assert rel_l2(num(x.grad), num(xc.grad)) < TOL
    assert rel_l2(num(sp.bias.grad), num(bc.grad)) < TOL
    if fac == "dense":
        assert rel_l2(num(sp.weight.grad), num(wc.grad)) < TOL
    else:
        for q, r in zip(sp.weight.parameters(), ref.parameters()):
            assert rel_l2(num(q.grad), num(r.grad)) < TOL


@pytest.mark.parametrize("name", golden_names("adamw_"))
def test_optimizer_matches_reference_trajectory(name):
    """neuraloperator_amd.AdamW (one fused launch per parameter) against the verbatim reference optimizer's
    parameter / exp_avg / exp_avg_sq trajectories, complex and real parameters."""
    import json
    from neuraloperator_amd import AdamW
    g = load_golden(name)
    kw = json.loads(str(g["kwargs"]))
    if "betas" in kw:
        kw["betas"] = tuple(kw["betas"])
    dev = torch.device("cuda:0")
    pc = torch.nn.Parameter(torch.from_numpy(g["pc0"]).to(dev))
    pr = torch.nn.Parameter(torch.from_numpy(g["pr0"]).to(dev))
    opt = AdamW([pc, pr], **kw)
    for t in range(int(g["steps"])):
        pc.grad = torch.from_numpy(g[f"gc_{t}"]).to(dev)
        pr.grad = torch.from_numpy(g[f"gr_{t}"]).to(dev)
        opt.step()
    tol = 2e-6
    assert rel_l2(pc.detach().cpu().numpy(), g["pc"]) < tol and rel_l2(pr.detach().cpu().numpy(), g["pr"]) < tol
    assert rel_l2(opt.state[pc]["exp_avg"].cpu().numpy(), g["m_c"]) < tol
    assert rel_l2(opt.state[pc]["exp_avg_sq"].cpu().numpy(), g["v_c"]) < tol
    assert rel_l2(opt.state[pr]["exp_avg_sq"].cpu().numpy(), g["v_r"]) < tol
    assert opt.state[pc]["exp_avg_sq"].dtype == torch.complex64 and opt.state[pc]["step"] == int(g["steps"])
    # Tensor-GaLore group (adamw.py:94-111, 139-196) on the device: low-rank moments, finite update, subspace kept
    wg = torch.nn.Parameter(torch.randn(8, 8, 12, 7, dtype=torch.cfloat, device=dev))
    w_before = wg.detach().clone()
    go = AdamW([pr], galore_params=[wg], galore_rank=0.25, lr=1e-2)
    for _ in range(2):
        wg.grad = torch.randn_like(wg)
        pr.grad = torch.randn_like(pr)
        go.step()
    st = go.state[wg]
    assert st["exp_avg"].shape != wg.shape and st["exp_avg"].is_cuda and st["step"] == 2
    assert torch.isfinite(torch.view_as_real(wg.detach())).all() and not torch.equal(wg.detach(), w_before)


@pytest.mark.parametrize("name", golden_names("galore_adamw_"))
def test_galore_group_matches_reference_trajectory(name):
    """The Tensor-GaLore group of neuraloperator_amd.AdamW on the GPU -- gradient projected onto the mode-wise subspaces and
    the update projected back as sc_modegemm launches (galore._engine_mode_dot, round 3) -- against the trajectory of the
    VERBATIM reference AdamW (training/adamw.py:94-111, 139-196; golden written by oracle/gen_golden.py).  The subspace
    (tensorly's Tucker is absent upstream-side here) is an input: the factors the golden run computed are loaded into
    the projector, so the optimizer arithmetic and the engine's mode products are what is compared."""
    import json
    from neuraloperator_amd import AdamW, galore
    g = load_golden(name)
    kw = json.loads(str(g["kwargs"]))
    rank = json.loads(str(g["rank"]))
    dev = torch.device("cuda:0")
    w = torch.nn.Parameter(torch.from_numpy(g["w0"]).to(dev))
    b = torch.nn.Parameter(torch.from_numpy(g["b0"]).to(dev))
    opt = AdamW([b], galore_params=[w], galore_rank=rank, **kw)
    proj = galore.TensorGaLoreProjector(rank=opt.galore_rank, update_proj_gap=opt.galore_update_proj_gap,
                                        scale=opt.galore_scale, activation_checkpoint=opt.activation_checkpoint,
                                        warm_restart=opt.warm_restart)
    proj.proj_tensor = [torch.from_numpy(g[f"proj_{d}"]).to(dev) for d in range(w.dim())]
    opt.state[w]["step"] = 0
    opt.state[w]["projector"] = proj
    tol = 5e-6
    for t in range(int(g["steps"])):
        w.grad = torch.from_numpy(g[f"gw_{t}"]).to(dev)
        b.grad = torch.from_numpy(g[f"gb_{t}"]).to(dev)
        opt.step()
        assert rel_l2(w.detach().cpu().numpy(), g[f"w_{t}"]) < tol, t
    st = opt.state[w]
    assert rel_l2(st["exp_avg"].cpu().numpy(), g["m"]) < tol and rel_l2(st["exp_avg_sq"].cpu().numpy(), g["v"]) < tol
    assert tuple(st["exp_avg"].shape) == tuple(g["m"].shape) != tuple(w.shape)
    assert rel_l2(b.detach().cpu().numpy(), g["b"]) < tol
    # the engine's mode products are the adjoint pair the projector needs
    x = torch.randn_like(w)
    low = proj.transform(proj.proj_tensor, x)
    y = torch.randn_like(low)
    lhs = torch.vdot(low.flatten(), y.flatten())
    rhs = torch.vdot(x.flatten(), proj.inverse_transform(proj.proj_tensor, y).flatten())
    assert abs(complex(lhs) - complex(rhs)) < 1e-3 * abs(complex(lhs))


def test_layer_step_is_graph_capturable():
    """A whole forward+backward of the layer records into a HIP graph (torch.cuda.CUDAGraph) and replays:
    every C-ABI call only enqueues work on the stream it is given -- no synchronisation, no allocation of
    its own after the first (warm-up) call has built the plan and the sub-block index table."""
    from neuraloperator_amd import SpectralConv
    dev = torch.device("cuda:0")
    torch.manual_seed(4)
    conv = SpectralConv(8, 8, (12, 12), max_n_modes=(16, 16)).to(dev)       # sub-block of a larger weight
    x = torch.randn(4, 8, 32, 32, device=dev, requires_grad=True)
    g = torch.randn(4, 8, 32, 32, device=dev)

    def step():
        y = conv(x)
        gx, gw, gb = torch.autograd.grad(y, (x, conv.weight.tensor, conv.bias), g)
        return y, gx, gw, gb

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            ref = step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    ref = [t.detach().clone() for t in ref]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    with torch.no_grad():
        x.copy_(torch.randn_like(x))            # new input, same buffers
    graph.replay()
    torch.cuda.synchronize()
    got = [t.detach().clone() for t in out]
    want = [t.detach() for t in step()]
    for a, b in zip(got, want):
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 1e-6
    assert rel_l2(got[0].cpu().numpy(), ref[0].cpu().numpy()) > 1e-3    # it really recomputed on the new input


@pytest.mark.parametrize("spatial,modes", [((128, 256), (32, 32)), ((24, 20), (8, 8)), ((8, 6, 10), (4, 4, 4))])
def test_fourier_layer_fused_epilogue(spatial, modes):
    """SURVEY.md 8 row f1, first step: out = gelu(conv(x) + skip) with the addition and the activation in the store
    path of the inverse transform (fused 2-D kernels) / one streaming pass behind it (other shapes), against the CPU
    oracle composition (reference: neuralop/layers/fno_block.py:392-414) -- output and the gradients of x, skip,
    weight and bias -- and against the module's own unfused composition."""
    from neuraloperator_amd import SpectralConv
    from oracle import spectral_oracle as so

    dev = torch.device("cuda:0")
    torch.manual_seed(12)
    conv = SpectralConv(6, 5, modes).to(dev)
    x = torch.randn(3, 6, *spatial)
    skip = torch.randn(3, 5, *spatial)
    g = torch.randn(3, 5, *spatial)
    xd, sd = x.to(dev).requires_grad_(True), skip.to(dev).requires_grad_(True)
    out = conv.forward_fused(xd, sd, "gelu")
    out.backward(g.to(dev))
    got = dict(out=out.detach(), gx=xd.grad, gskip=sd.grad, gw=conv.weight.tensor.grad.clone(),
               gb=conv.bias.grad.clone())
    xr, sr = x.clone().requires_grad_(True), skip.clone().requires_grad_(True)
    wr = conv.weight.tensor.detach().cpu().requires_grad_(True)
    br = conv.bias.detach().cpu().requires_grad_(True)
    ref = torch.nn.functional.gelu(so.forward_torch(xr, wr, br, conv.n_modes, conv.max_n_modes) + sr)
    ref.backward(g)
    want = dict(out=ref.detach(), gx=xr.grad, gskip=sr.grad, gw=wr.grad, gb=br.grad)
    for k in got:
        assert rel_l2(got[k].cpu().numpy(), want[k].numpy()) < TOL, k
    conv.zero_grad()
    x2, s2 = x.to(dev).requires_grad_(True), skip.to(dev).requires_grad_(True)
    torch.nn.functional.gelu(conv(x2) + s2).backward(g.to(dev))
    assert rel_l2(xd.grad.cpu().numpy(), x2.grad.cpu().numpy()) < TOL
    # no activation: plain sum
    with torch.no_grad():
        y_lin = conv.forward_fused(xd.detach(), sd.detach(), None)
        assert rel_l2(y_lin.cpu().numpy(), (conv(xd.detach()) + sd.detach()).cpu().numpy()) < TOL


@pytest.mark.parametrize("kept,n_img,mode", [((256, 129), 6, "adjoint"), ((101, 129), 3, "padded")])
def test_two_pass_row_kernel_adds_the_epilogue_skip_on_device(lib, kept, n_img, mode):
    """Round 6: at 1024-point rows with 129 kept columns (configs[4]) the SC_ACT_NONE addend of sc_transform_inverse_ex rides
    in the store path of k_f2p_c2r_w1024<true> (the block backward's gradient around the spectral convolution): bit for bit
    the plain transform followed by the sum (the same two additions in the same order); both inverse modes, several images
    (the chunked host loop offsets the addend with the output)."""
    from neuraloperator_amd import _lib
    dev = torch.device("cuda:0")
    torch.manual_seed(33)
    spatial = (1024, 1024)
    md = _lib.SC_INV_PADDED if mode == "padded" else _lib.SC_INV_ADJ_R2C
    plan = lib.plan_create(list(spatial), list(kept), fft_norm="forward", flags=0)
    try:
        ws = torch.empty(max(lib.plan_workspace_bytes(plan, n_img), 256), dtype=torch.uint8, device=dev)
        yhat = torch.randn(n_img, *kept, 2, device=dev)
        bias = torch.randn(n_img, device=dev) if mode == "padded" else None
        bp = 0 if bias is None else bias.data_ptr()
        skip = torch.randn(n_img, *spatial, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        plain = torch.full((n_img, *spatial), float("nan"), device=dev)
        lib.transform_inverse(plan, md, yhat.data_ptr(), bp, n_img, plain.data_ptr(), n_img, ws.data_ptr(), st)
        fused = torch.full((n_img, *spatial), float("nan"), device=dev)
        lib.transform_inverse_ex(plan, md, yhat.data_ptr(), bp, n_img, skip.data_ptr(), 0, _lib.SC_ACT_NONE,
                                 fused.data_ptr(), n_img, ws.data_ptr(), st)
        torch.cuda.synchronize()
        assert torch.equal(fused, plain + skip)
    finally:
        lib.plan_destroy(plan)


def test_one_activation_on_every_route_bit_for_bit(lib):
    """sc_gelu (sc_device.h) is evaluated by the fused store path of the 2-D inverse transform (scalar form), by the
    streaming k_epilogue pass behind the other transforms (scalar form) and by the pointwise kernels (PAIR form on packed
    fp32 instructions, round 6): the same IEEE operations in the same order -> the same bits for the same argument.
    Every route is made to compute gelu(0 + s): a zero spectrum under the two transform routes, a zero weight and a unit
    gate in the 1 x 1 map."""
    from neuraloperator_amd import _lib
    dev = torch.device("cuda:0")
    torch.manual_seed(41)
    B, C = 2, 32
    s = (torch.randn(B, C, 4096, device=dev) * 3.0).contiguous()
    s.view(-1)[:8] = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 6.5, -6.5, 40.0, -40.0], device=dev)
    st = torch.cuda.current_stream().cuda_stream
    outs = {}
    for tag, spatial, kept in (("fused 2-D store path", (64, 64), (16, 9)), ("k_epilogue pass", (16, 16, 16), (4, 4, 3))):
        plan = lib.plan_create(list(spatial), list(kept), fft_norm="forward", flags=0)
        try:
            ws = torch.empty(max(lib.plan_workspace_bytes(plan, B * C), 256), dtype=torch.uint8, device=dev)
            yhat = torch.zeros(B * C, *kept, 2, device=dev)
            y = torch.full((B, C, 4096), float("nan"), device=dev)
            lib.transform_inverse_ex(plan, _lib.SC_INV_PADDED, yhat.data_ptr(), 0, C, s.data_ptr(), 0, _lib.SC_ACT_GELU,
                                     y.data_ptr(), B * C, ws.data_ptr(), st)
            outs[tag] = y
        finally:
            lib.plan_destroy(plan)
    w = torch.zeros(C, C, device=dev)
    gate = torch.ones(C, device=dev)
    x = torch.randn(B, C, 4096, device=dev)
    y = torch.full((B, C, 4096), float("nan"), device=dev)
    lib.pointwise_linear_forward_ex(B, C, C, 4096, _lib.SC_PLX_ACT, x.data_ptr(), w.data_ptr(), 0, s.data_ptr(), gate.data_ptr(),
                                    y.data_ptr(), 0, st)
    outs["1 x 1 map (pair form)"] = y
    torch.cuda.synchronize()
    ref = torch.nn.functional.gelu(s.double()).float()
    tags = list(outs)
    for t in tags:
        assert torch.isfinite(outs[t]).all(), t
        assert rel_l2(outs[t].cpu().numpy(), ref.cpu().numpy()) < 1e-6, t
    for t in tags[1:]:
        assert torch.equal(outs[t].view(torch.int32), outs[tags[0]].view(torch.int32)), (tags[0], t)


@pytest.mark.parametrize("chans", [(32, 32, 32), (64, 32, 64), (64, 64, 64), (128, 64, 128)], ids=str)
def test_pointwise_mlp_pass(chans):
    # (128, 64, 128) has the forward kernel only: with gradients it takes the composition, checked like the others
    """sc_pointwise_mlp_forward / _backward (ChannelMLP + soft-gating skip + closing GELU in one
    pass) through neuraloperator_amd.blocks.fused_channel_mlp against torch autograd of the float64 composition."""
    import torch.nn.functional as F
    from neuraloperator_amd.blocks import fused_channel_mlp
    ci, ch, co = chans
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(ci + ch)
    mk = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc)
    x, sk, go = mk(3, ci, 24, 40), mk(3, co, 24, 40), mk(3, co, 24, 40)          # 960 pixels per sample
    w1, b1, w2, b2, gt = mk(ch, ci, 1, sc=ci ** -0.5), mk(ch), mk(co, ch, 1, sc=ch ** -0.5), mk(co), mk(1, co, 1, 1)
    import pointwise_reference as pr
    ref, grads = pr.grads64(lambda *a: pr.mlp64(*a, act=1), (x, w1, b1, w2, b2, sk, gt), go)   # the float64 composition
    dl = [t.to(dev).requires_grad_(True) for t in (x, w1, b1, w2, b2, sk, gt)]
    with torch.no_grad():                                      # inference: every shape has the forward kernel
        out_ng = fused_channel_mlp(dl[0], dl[1], dl[2], dl[3], dl[4], skip_src=dl[5], gate=dl[6], activation="gelu")
    assert rel_l2(out_ng.cpu().numpy(), ref.detach().numpy()) < TOL
    out = fused_channel_mlp(dl[0], dl[1], dl[2], dl[3], dl[4], skip_src=dl[5], gate=dl[6], activation="gelu")
    out.backward(go.to(dev))
    assert rel_l2(out.detach().cpu().numpy(), ref.detach().numpy()) < TOL
    for a, b in zip(dl, grads):
        assert rel_l2(a.grad.cpu().numpy(), b.numpy()) < TOL


def _block_oracle(blk, x, g, index):
    """fno_block.py:377-414 (defaults: linear fno skip, soft-gating MLP skip, ChannelMLP, GELU, post-activation) on
    the CPU: oracle.forward_torch for the convolution, ATen for the pointwise ops, autograd for every gradient."""
    import torch.nn.functional as F
    from oracle import spectral_oracle as so
    P = {n: q.detach().cpu().clone().requires_grad_(True) for n, q in blk.named_parameters()}
    xc = x.detach().cpu().clone().requires_grad_(True)
    s = list(xc.shape)
    flat = lambda t: t.reshape(s[0], t.shape[1], -1)
    pre = bool(getattr(blk, "preactivation", False))                    # fno_block.py:416-458 instead of :377-414
    xin = F.gelu(xc) if pre else xc
    x_skip_fno = F.conv1d(flat(xin), P[f"fno_skips.{index}.conv.weight"]).reshape(s)
    x_skip_mlp = P[f"channel_mlp_skips.{index}.weight"] * xin
    nm = list(blk.convs[index].n_modes)
    t = so.forward_torch(xin, P[f"convs.{index}.weight.tensor"], P[f"convs.{index}.bias"], nm, nm) + x_skip_fno
    if index < blk.n_layers - 1:
        t = F.gelu(t)
    h = F.gelu(F.conv1d(flat(t), P[f"channel_mlp.{index}.fcs.0.weight"], P[f"channel_mlp.{index}.fcs.0.bias"]))
    t = F.conv1d(h, P[f"channel_mlp.{index}.fcs.1.weight"], P[f"channel_mlp.{index}.fcs.1.bias"]).reshape(s) + x_skip_mlp
    if index < blk.n_layers - 1 and not pre:
        t = F.gelu(t)
    t.backward(g.detach().cpu())
    return t.detach(), xc.grad, {n: q.grad for n, q in P.items() if q.grad is not None}


@pytest.mark.parametrize("pre", [False, True], ids=["postactivation", "preactivation"])
def test_fused_block_forward_matches_op_sequence(pre):
    """A whole FNO block through the two fused passes against the reference's op sequence evaluated by the CPU ORACLE
    on the same parameters (stand-in module with FNOBlocks' attribute surface; the verbatim class is checked on the
    CPU tier) -- and, as a second check, against the unfused op sequence on the GPU.  Pre-activation blocks
    (fno_block.py:416-458; session 2) run the same engine passes composed by autograd."""
    from block_standin import Blocks
    from neuraloperator_amd import blocks as nb
    dev = torch.device("cuda:0")
    torch.manual_seed(4)
    blk = Blocks(64, (16, 16), preactivation=pre).to(dev)
    with torch.no_grad():
        for q in blk.parameters():
            if q.is_complex():
                q.mul_(4.0)
        blk.channel_mlp_skips[0].weight.copy_(torch.randn_like(blk.channel_mlp_skips[0].weight))
    x = torch.randn(4, 64, 64, 64, device=dev)
    g = torch.randn(4, 64, 64, 64, device=dev)
    for index in (0, 1):
        res = []
        for fn in (lambda t: blk(t, index), lambda t: nb.fused_block_forward(blk, t, index)):
            blk.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(True)
            y = fn(xi)
            y.backward(g)
            res.append((y.detach(), xi.grad.clone(), {n: q.grad.clone() for n, q in blk.named_parameters() if q.grad is not None}))
        yo, gxo, gpo = _block_oracle(blk, x, g, index)
        for y1, gx1, gp1 in res:                              # both GPU routes against the oracle
            assert rel_l2(y1.cpu().numpy(), yo.numpy()) < TOL and rel_l2(gx1.cpu().numpy(), gxo.numpy()) < TOL
            assert set(gpo) == set(gp1)
            for n in gpo:
                a, b = gp1[n].cpu(), gpo[n]
                a, b = (torch.view_as_real(a), torch.view_as_real(b)) if a.is_complex() else (a, b)
                assert rel_l2(a.numpy(), b.numpy()) < 2e-5, n


@pytest.mark.parametrize("hidden,expansion", [(128, 0.5), (128, 1.0), (64, 2.0)], ids=["128-64-128", "128-128-128", "64-128-64"])
def test_fused_block_hidden_128_matches_the_oracle(hidden, expansion):
    """a configs[4]-width block (128 channels; also hidden 128) as ONE autograd node on the two-pass engine
    form (csrc/sc_kernels_plinx.h) against the reference's op sequence evaluated by the CPU oracle -- output, input gradient
    and every parameter gradient, first and last block.  (The unfused op sequence is not run on the GPU here: F.conv1d's
    fp32 backward at 128 channels lands on MIOpen's naive kernels, 338 ms per call -- profiles/r06_block128_before.txt.)"""
    from block_standin import Blocks
    from neuraloperator_amd import blocks as nb
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    blk = Blocks(hidden, (12, 12), expansion=expansion).to(dev)
    with torch.no_grad():
        for q in blk.parameters():
            if q.is_complex():
                q.mul_(4.0)
        for i in (0, 1):
            blk.channel_mlp_skips[i].weight.copy_(torch.randn_like(blk.channel_mlp_skips[i].weight))
    x = torch.randn(2, hidden, 32, 48, device=dev)
    g = torch.randn(2, hidden, 32, 48, device=dev)
    for index in (0, 1):
        nodes = []
        orig = nb.FusedBlockFn.apply
        nb.FusedBlockFn.apply = staticmethod(lambda *a: (nodes.append(1), orig(*a))[1])
        try:
            blk.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(True)
            y = nb.fused_block_forward(blk, xi, index)
            y.backward(g)
        finally:
            nb.FusedBlockFn.apply = orig
        assert nodes == [1]
        gp1 = {n: q.grad.clone() for n, q in blk.named_parameters() if q.grad is not None}
        yo, gxo, gpo = _block_oracle(blk, x, g, index)
        assert rel_l2(y.detach().cpu().numpy(), yo.numpy()) < TOL and rel_l2(xi.grad.cpu().numpy(), gxo.numpy()) < TOL
        assert set(gpo) == set(gp1)
        for n in gpo:
            a, b = gp1[n].cpu(), gpo[n]
            a, b = (torch.view_as_real(a), torch.view_as_real(b)) if a.is_complex() else (a, b)
            assert rel_l2(a.numpy(), b.numpy()) < 2e-5, n


@pytest.mark.parametrize("ci,ch,co", [(128, 64, 128), (128, 128, 128), (32, 128, 64)], ids=str)
def test_two_pass_channel_mlp_and_rectangular_linear_maps(ci, ch, co):
    """blocks.fused_channel_mlp on channel counts without a one-pass kernel (PointwiseMLP2Fn: two engine passes each way)
    and blocks.fused_linear on a rectangular map (PointwiseLinearXFn) against torch autograd in float64."""
    import torch.nn.functional as F
    from neuraloperator_amd import blocks as nb
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(ci + ch)
    B, H, W = 3, 24, 40
    x, skip, go = torch.randn(B, ci, H, W, generator=g), torch.randn(B, co, H, W, generator=g), torch.randn(B, co, H, W, generator=g)
    w1, b1 = torch.randn(ch, ci, 1, generator=g) / ci ** 0.5, torch.randn(ch, generator=g)
    w2, b2 = torch.randn(co, ch, 1, generator=g) / ch ** 0.5, torch.randn(co, generator=g)
    gate = torch.randn(1, co, 1, 1, generator=g)
    import pointwise_reference as pr
    ref, grads = pr.grads64(lambda *a: pr.mlp64(*a, act=1), (x, w1, b1, w2, b2, skip, gate), go)
    dl = [t.to(dev).requires_grad_(True) for t in (x, w1, b1, w2, b2, skip, gate)]
    seen = []
    orig = nb.PointwiseMLP2Fn.apply
    nb.PointwiseMLP2Fn.apply = staticmethod(lambda *a: (seen.append(1), orig(*a))[1])
    try:
        out = nb.fused_channel_mlp(dl[0], dl[1], dl[2], dl[3], dl[4], skip_src=dl[5], gate=dl[6], activation="gelu")
    finally:
        nb.PointwiseMLP2Fn.apply = orig
    assert seen == [1]
    out.backward(go.to(dev))
    assert rel_l2(out.detach().cpu().numpy(), ref.detach().numpy()) < TOL
    for a, b in zip(dl, grads):
        assert rel_l2(a.grad.cpu().numpy(), b.numpy()) < TOL
    # rectangular 1 x 1 map
    xl, wl, bl = (t.to(dev).requires_grad_(True) for t in (x, w1, b1))
    o2 = nb.fused_linear(xl, wl, bl)
    r2 = pr.linear64(x, w1, b1)
    assert o2.grad_fn is not None and "PointwiseLinear" in type(o2.grad_fn).__name__
    assert rel_l2(o2.detach().cpu().numpy(), r2.numpy()) < TOL


@pytest.mark.parametrize("c", [32, 64])
def test_pointwise_linear_pass(c):
    """The block's 1 x 1 linear skip (k_plin_fwd / k_plin_bwd) through blocks.fused_linear against torch float64."""
    from neuraloperator_amd.blocks import fused_linear
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(c)
    x, go = torch.randn(3, c, 24, 40, generator=g), torch.randn(3, c, 24, 40, generator=g)
    w, b = torch.randn(c, c, 1, generator=g) / c ** 0.5, torch.randn(c, generator=g)
    import pointwise_reference as pr
    ref, grads = pr.grads64(pr.linear64, (x, w, b), go)
    xg, wg, bg = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    out = fused_linear(xg, wg, bg)
    out.backward(go.to(dev))
    assert rel_l2(out.detach().cpu().numpy(), ref.numpy()) < TOL
    for a, r in zip((xg, wg, bg), grads):
        assert rel_l2(a.grad.cpu().numpy(), r.numpy()) < TOL


@pytest.mark.parametrize("grid", ["equiangular", "legendre-gauss"])
def test_spherical_conv_on_device(grid):
    """SphericalConv (last item) on the GPU against the float64 restatement of its definition
    (tests/test_spherical.py; torch_harmonics itself is absent: parity with it is unpinned)."""
    from neuraloperator_amd import SphericalConv
    from test_spherical import _ref_isht, _ref_sht
    dev = torch.device("cuda:0")
    torch.manual_seed(2)
    conv = SphericalConv(4, 5, (12, 24), factorization=None, sht_grids=grid).to(dev)
    with torch.no_grad():
        conv.weight.tensor.mul_(3.0)
    x = torch.randn(2, 4, 25, 48)
    g = torch.randn(2, 5, 25, 48)
    xi = x.to(dev).requires_grad_(True)
    y = conv(xi)
    y.backward(g.to(dev))
    xd = x.double().requires_grad_(True)
    w = conv.weight.tensor.detach().cpu().to(torch.complex128).requires_grad_(True)
    b = conv.bias.detach().cpu().double().requires_grad_(True)
    yh = torch.einsum("bilm,iol->bolm", _ref_sht(xd, 12, 12, "ortho", grid), w)
    yr = _ref_isht(yh, 25, 48, "ortho", grid) + b
    yr.backward(g.double())
    assert rel_l2(y.detach().cpu().numpy(), yr.detach().numpy()) < TOL
    assert rel_l2(xi.grad.cpu().numpy(), xd.grad.numpy()) < TOL
    assert rel_l2(torch.view_as_real(conv.weight.tensor.grad).cpu().numpy(), torch.view_as_real(w.grad).numpy()) < 2e-5
    assert rel_l2(conv.bias.grad.cpu().numpy(), b.grad.numpy()) < TOL
