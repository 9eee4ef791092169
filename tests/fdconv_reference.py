"""float64 restatement of the finite-difference convolution (neuralop/layers/differential_conv.py) for the tests: the
folded weights, F.pad and F.convNd on the host, the case table the recorder and the tests share, and a loader of the
verbatim class.  torch on the host, no engine."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PAD_MODE = {"periodic": "circular", "zeros": "constant", "replicate": "replicate", "reflect": "reflect"}
# tile constants of sc_kernels_fdconv.h the extents are cut against: general route 16 x 64, matrix-core route 4 x 32
FD_TR, FD_TC, FDM_TR, FDM_TC = 16, 64, 4, 32
GENERAL, MFMA = 1, 2


def folded_weight(w, grid_width):
    """W'[.., t] = W[.., t] / h off the centre, W'[.., centre] = -(sum of the other taps) / h"""
    flat = w.reshape(*w.shape[:2], -1)
    c = flat.shape[-1] // 2
    off = torch.cat([flat[..., :c], flat[..., c + 1:]], -1)
    out = flat.clone()
    out[..., c] = -off.sum(-1)
    return (out / grid_width).reshape(w.shape)


def fdconv(x, w, grid_width, groups=1, padding="periodic"):
    """the layer as ONE convolution of the padded input with the folded weights, in the dtype of its inputs"""
    nd, r = x.dim() - 2, w.shape[-1] // 2
    xp = F.pad(x, [r, r] * nd, mode=PAD_MODE[padding])
    return getattr(F, f"conv{nd}d")(xp, folded_weight(w, grid_width), groups=groups)


def fdconv_with_grads(x, w, g, grid_width, groups, padding):
    """(out, gx, gw) of the helper in float64 for fp32 or float64 host tensors"""
    x64, w64 = x.detach().double().cpu().requires_grad_(True), w.detach().double().cpu().requires_grad_(True)
    out = fdconv(x64, w64, grid_width, groups, padding)
    out.backward(g.detach().double().cpu())
    return out.detach(), x64.grad, w64.grad


def formula_fp32(x, w, g, grid_width, groups, padding):
    """(out, gx, gw) of the reference's formula as it stands -- the padded k^d convolution, the 1 x 1 convolution of the
    summed kernel, the subtraction and the division -- in fp32 with torch on the host"""
    x32, w32 = x.detach().float().cpu().requires_grad_(True), w.detach().float().cpu().requires_grad_(True)
    nd, r = x32.dim() - 2, w32.shape[-1] // 2
    conv = getattr(F, f"conv{nd}d")
    full = conv(F.pad(x32, [r, r] * nd, mode=PAD_MODE[padding]), w32, groups=groups)
    centre = conv(x32, w32.sum(dim=tuple(range(2, 2 + nd)), keepdim=True), groups=groups)
    out = (full - centre) / grid_width
    out.backward(g.detach().float().cpu())
    return out.detach().numpy(), x32.grad.numpy(), w32.grad.numpy()


def smooth_bars(x, w, g, grid_width, groups, padding, want):
    """the bar of a smooth-field case without a record: twice the error of the reference's formula in fp32 (torch on the
    host) against the float64 helper `want`"""
    return tuple(2.0 * rel_l2(a, b) for a, b in zip(formula_fp32(x, w, g, grid_width, groups, padding), want))


def magnitudes(x, w, g, grid_width, groups, padding):
    """(out, gx, gw) of conv_pad(|x|, |W|) / h with cotangent |g| in float64: the size of the terms the layer's
    difference is formed from.  An error is measured against these where the exact result is identically zero (a
    periodic axis of extent 1: every tap reads the same point and the folded weights sum to zero)."""
    x64 = x.detach().double().cpu().abs().requires_grad_(True)
    w64 = w.detach().double().cpu().abs().requires_grad_(True)
    nd, r = x64.dim() - 2, w64.shape[-1] // 2
    out = getattr(F, f"conv{nd}d")(F.pad(x64, [r, r] * nd, mode=PAD_MODE[padding]), w64, groups=groups) / grid_width
    out.backward(g.detach().double().cpu().abs())
    return out.detach().numpy(), x64.grad.numpy(), w64.grad.numpy()


def rel_l2(a, b, zero_scale=None):
    """|a - b| / |b|; where zero_scale is given and b is zero up to float64 round-off of its terms (|b| <= 1e-12
    |zero_scale|: the exact result is identically zero), |a - b| / |zero_scale|"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    den = np.linalg.norm(b.ravel())
    if zero_scale is not None:
        zs = np.linalg.norm(np.asarray(zero_scale, np.float64).ravel())
        if den <= 1e-12 * zs:
            den = zs
    return float(np.linalg.norm((a - b).ravel()) / max(den, 1e-300))


# ---- cases: name -> dict(dims, c_in, c_out, groups, k, padding, batch, route, smooth) ----------------------------------
def _case(dims, c_in, c_out, groups=1, k=3, padding="periodic", batch=2, route=GENERAL, smooth=False):
    return dict(dims=tuple(dims), c_in=c_in, c_out=c_out, groups=groups, k=k, padding=padding, batch=batch, route=route,
                smooth=smooth)


# Recorded cases (tests/record_fdconv.py writes tests/golden/fdconv_<name>.npz).  Three of the issue's extents are
# smaller here, because a committed file may hold 1 MiB at most and the float64 record of (2, 32, 13, 70) alone is
# 1.4 MiB: depthwise 9 x 70 -> 3 x 70 (still one full 64-column tile and a remainder of 6; 9 rows crossed no tile of 16
# either), matrix-core 13 x 70 -> 5 x 38 (one full 4 x 32 tile and a remainder on both axes), smooth 32 x 32 -> 16 x 16
# (grid_width 1 / 16).  The planned extents run against the float64 helper in LIVE_CASES below, on both tiers: the two
# random ones at 1e-5, the smooth 32 x 32 field at twice the error of the reference's formula in fp32 (smooth_bars).
CASES = {
    "1d_k3_periodic_g2": _case((9,), 4, 6, groups=2),
    "1d_k5_reflect_depthwise": _case((7,), 3, 3, groups=3, k=5, padding="reflect"),
    "1d_k7_zeros_short": _case((4,), 5, 2, k=7, padding="zeros"),
    "1d_k3_periodic_n1": _case((1,), 2, 3),
    "1d_k3_periodic_n2": _case((2,), 2, 3),
    "2d_k3_replicate_g2": _case((5, 9), 6, 4, groups=2, padding="replicate"),
    "2d_k5_reflect": _case((6, 7), 3, 3, k=5, padding="reflect"),
    "2d_k3_periodic_depthwise32": _case((3, 70), 32, 32, groups=32),
    "2d_k3_periodic_1x4": _case((1, 4), 5, 7),
    "2d_k3_zeros_33_31": _case((8, 8), 33, 31, padding="zeros"),
    "2d_mfma_periodic_32": _case((5, 38), 32, 32, route=MFMA),
    "2d_mfma_zeros_32_b1": _case((8, 8), 32, 32, padding="zeros", batch=1, route=MFMA),
    "3d_k3_periodic": _case((5, 6, 7), 4, 4),
    "3d_k3_zeros_depthwise": _case((4, 5, 6), 3, 3, groups=3, padding="zeros"),
    "3d_k3_reflect": _case((4, 3, 5), 2, 3, padding="reflect"),
    "3d_k5_replicate": _case((3, 6, 5), 2, 2, k=5, padding="replicate"),
    "2d_smooth_periodic_32": _case((16, 16), 32, 32, route=MFMA, smooth=True),
}
# not recorded (too large to commit): checked against the float64 helper on the host, see above for the bars
LIVE_CASES = {
    "2d_k3_periodic_depthwise32_9x70": _case((9, 70), 32, 32, groups=32),
    "2d_mfma_periodic_32_13x70": _case((13, 70), 32, 32, route=MFMA),
    "2d_smooth_periodic_32x32": _case((32, 32), 32, 32, route=MFMA, smooth=True),
}


# Kernel-edge cases: free-standing descriptors at the tile, chunk and route edges of sc_kernels_fdconv.h, run on the
# device by tests/test_gpu_fdconv_kernels.py (the float64 helper is the reference); EMU_KERNEL_CASES names those the
# one-thread-per-lane emulation finishes in a few seconds.  Groups are lettered as in that file's docstring.
def _kernel_cases():
    modes = ("periodic", "zeros", "replicate", "reflect")
    c = {}
    for k in (3, 5, 7):                                      # a: one past FD_TR and FD_TC (and FD_OCB), every mode
        for m in modes:
            c[f"a_17x65_k{k}_{m}"] = _case((17, 65), 2, 5, k=k, padding=m)
    for m in ("replicate", "reflect"):                       # a point and its high pad in different tiles on both axes
        c[f"a_33x130_k7_{m}"] = _case((33, 130), 2, 5, k=7, padding=m, batch=1)
    for m in ("replicate", "reflect"):                       # b: d + 2 r crosses a tile, d does not
        c[f"b_11x59_k7_{m}"] = _case((11, 59), 2, 3, k=7, padding=m)
        c[f"b_16x64_k3_{m}"] = _case((16, 64), 2, 3, k=3, padding=m)
    c["c_reflect_k7_4x4"] = _case((4, 4), 2, 3, k=7, padding="reflect")          # c: smallest legal extents
    c["c_reflect_k5_3"] = _case((3,), 2, 3, k=5, padding="reflect")
    c["c_periodic_k7_3x3"] = _case((3, 3), 2, 3, k=7)
    c["c_periodic_k5_2x70"] = _case((2, 70), 2, 3, k=5)
    c["c_periodic_k3_1x65"] = _case((1, 65), 2, 3, k=3)
    for m in modes:                                          # d: three axes
        c[f"d_3x17x65_k3_{m}"] = _case((3, 17, 65), 2, 3, k=3, padding=m)
    c["d_2x5x6_k5_zeros"] = _case((2, 5, 6), 2, 3, k=5, padding="zeros")
    c["d_2x5x6_k5_replicate"] = _case((2, 5, 6), 2, 3, k=5, padding="replicate")
    c["d_7x4x4_k7_reflect"] = _case((7, 4, 4), 2, 3, k=7, padding="reflect")     # reflect needs extents above k / 2 = 3
    for og in (3, 4, 5):                                     # e: output channels of a group around FD_OCB
        c[f"e_cout_g{og}_groups1"] = _case((5, 9), 2, og)
        c[f"e_cout_g{og}_groups2"] = _case((5, 9), 4, 2 * og, groups=2, padding="reflect")
    c["e_depthwise5"] = _case((5, 9), 5, 5, groups=5, padding="zeros")
    c["f_one_chunk_33_31"] = _case((17, 65), 33, 31, batch=1)                    # f: 1023 jobs, 1024 / jobs = 1 chunk
    c["f_one_chunk_33_32"] = _case((17, 65), 33, 32, batch=1)                    # 1056 jobs >= 1024: the other branch
    c["f_704_batch3_empty_chunks"] = _case((704,), 2, 2, batch=3)                # 33 units, 32 chunks of 2: 17.. are empty
    c["f_704_batch1"] = _case((704,), 2, 2, batch=1)                             # 11 units, 11 chunks
    for ci in (32, 64, 128):                                 # g: matrix cores, one past FDM_TR and FDM_TC
        for co in (32, 64, 128):
            for m in ("periodic", "zeros"):
                c[f"g_mfma_{ci}_{co}_{m}"] = _case((5, 33), ci, co, padding=m, batch=1, route=MFMA)
    c["g_mfma_32_32_1x31"] = _case((1, 31), 32, 32, padding="zeros", batch=1, route=MFMA)
    c["g_mfma_32_32_4x32"] = _case((4, 32), 32, 32, padding="zeros", batch=1, route=MFMA)
    c["g_mfma_32_32_periodic_2x2"] = _case((2, 2), 32, 32, batch=1, route=MFMA)
    c["g_mfma_32_32_49x129_65_units"] = _case((49, 129), 32, 32, batch=1, route=MFMA)   # 64 chunks of 2, 33 carry data
    return c


KERNEL_CASES = _kernel_cases()
EMU_KERNEL_CASES = ("b_16x64_k3_replicate", "b_16x64_k3_reflect", "c_reflect_k7_4x4", "c_reflect_k5_3",
                    "c_periodic_k7_3x3", "c_periodic_k5_2x70", "c_periodic_k3_1x65", "d_2x5x6_k5_zeros",
                    "d_2x5x6_k5_replicate")


def grid_width_of(cfg):
    return 1.0 / cfg["dims"][-1]


def smooth_field(batch, channels, dims):
    """products of sines and cosines of wavenumber 1..3 per axis, fp32"""
    axes = [torch.arange(n, dtype=torch.float64) * (2 * np.pi / n) for n in dims]
    x = torch.empty(batch, channels, *dims, dtype=torch.float64)
    for b in range(batch):
        for c in range(channels):
            v = torch.ones(dims, dtype=torch.float64)
            for a, t in enumerate(axes):
                kx = 1 + (b + c + a) % 3
                f = torch.sin(kx * t + 0.3 * c) if (c + a) % 2 else torch.cos(kx * t - 0.2 * b)
                v = v * f.reshape([-1 if i == a else 1 for i in range(len(dims))])
            x[b, c] = v
    return x.float()


def case_inputs(cfg, seed):
    """fp32 input, weight (the initialisation of torch's ConvNd under the seed) and cotangent of a case"""
    g = torch.Generator().manual_seed(seed)
    nd = len(cfg["dims"])
    if cfg["smooth"]:
        x = smooth_field(cfg["batch"], cfg["c_in"], cfg["dims"])
    else:
        x = torch.randn(cfg["batch"], cfg["c_in"], *cfg["dims"], generator=g, dtype=torch.float32)
    fan_in = (cfg["c_in"] // cfg["groups"]) * cfg["k"] ** nd
    bound = 1.0 / np.sqrt(fan_in)                             # kaiming_uniform_(a = sqrt 5), ConvNd.reset_parameters
    w = (torch.rand(cfg["c_out"], cfg["c_in"] // cfg["groups"], *([cfg["k"]] * nd), generator=g,
                    dtype=torch.float32) * 2 - 1) * bound
    gout = torch.randn(cfg["batch"], cfg["c_out"], *cfg["dims"], generator=g, dtype=torch.float32)
    return x, w, gout


def module_kwargs(cfg):
    return dict(in_channels=cfg["c_in"], out_channels=cfg["c_out"], n_dim=len(cfg["dims"]), kernel_size=cfg["k"],
                groups=cfg["groups"], padding=cfg["padding"])


def run_module(cfg, x, w, gout, grid_width, device):
    """neuraloperator_amd.FiniteDifferenceConvolution forward + backward: (out, gx, gw, module) as host numpy arrays"""
    from neuraloperator_amd import FiniteDifferenceConvolution
    m = FiniteDifferenceConvolution(**module_kwargs(cfg))
    with torch.no_grad():
        m.weight.copy_(w)
    m = m.to(device)
    xd = x.to(device).clone().requires_grad_(True)
    assert m.on_engine(xd, grid_width)
    out = m(xd, grid_width)
    out.backward(gout.to(device))
    return out.detach().cpu().numpy(), xd.grad.cpu().numpy(), m.weight.grad.cpu().numpy(), m


def centre_index(cfg):
    return (slice(None), slice(None)) + (cfg["k"] // 2,) * len(cfg["dims"])


def check_against(cfg, got, want, bars, zero_scales=(None, None, None)):
    """got / want = (out, gx, gw); bars = the three rel-L2 bounds; zero_scales = magnitudes(..) for a case whose exact
    result may be identically zero.  Returns the measured errors."""
    errs = tuple(rel_l2(a, b, z) for a, b, z in zip(got, want, zero_scales))
    for name, e, bar in zip(("out", "grad:x", "grad:weight"), errs, bars):
        assert e <= bar, (name, e, bar)
    assert not got[2][centre_index(cfg)].any(), "the centre tap's weight gradient is exactly 0"
    return errs


def record_bars(cfg, rec):
    """1e-5 for every layer of the project; on the smooth field, where the stencil cancels, twice the verbatim fp32
    class's own error against its float64 run"""
    if cfg["smooth"]:
        return tuple(2.0 * float(rec["f32err:" + k]) for k in ("out", "grad:x", "grad:weight"))
    return (1e-5, 1e-5, 1e-5)


# ---- free-standing descriptors through the C-ABI (the emulation and the GPU tier run the same runner) ------------------
def desc_of(cfg, h):
    from neuraloperator_amd import _lib
    return _lib.ScEngineLib.fdconv_desc(dims=cfg["dims"], batch=cfg["batch"], c_in=cfg["c_in"], c_out=cfg["c_out"],
                                        k=cfg["k"], groups=cfg["groups"], padding=cfg["padding"], inv_h=1.0 / h)


def run_descriptor(lib, cfg, x, w, g, h, want_x=True, want_w=True, device="cpu", stream=0):
    """sc_fdconv_forward + sc_fdconv_backward on tensors moved to `device`: (out, gx, gw) on the host"""
    x, w, g = (t.to(device) for t in (x, w, g))
    d = desc_of(cfg, h)
    nbytes, fbytes = lib.fdconv_workspace_bytes(d), lib.fdconv_forward_workspace_bytes(d)
    assert 0 < fbytes <= nbytes
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    y = torch.full((cfg["batch"], cfg["c_out"], *cfg["dims"]), float("nan"), device=device)
    lib.fdconv_forward(d, x.data_ptr(), w.data_ptr(), y.data_ptr(), ws.data_ptr(), fbytes, stream)  # its own, smaller size
    gx = torch.full_like(x, float("nan")) if want_x else None
    gw = torch.full_like(w, float("nan")) if want_w else None
    ws.fill_(0xff)                                           # the backward call owes nothing to the forward call's workspace
    lib.fdconv_backward(d, x.data_ptr(), w.data_ptr(), g.data_ptr(), 0 if gx is None else gx.data_ptr(),
                        0 if gw is None else gw.data_ptr(), ws.data_ptr(), nbytes, stream)
    return tuple(None if t is None else t.cpu() for t in (y, gx, gw))


# ---- per-element bound: |got - want| <= gamma_N A ----------------------------------------------------------------------
U = 2.0 ** -24                                               # unit round-off of fp32


def gamma(n):
    return n * U / (1.0 - n * U)


def wgrad_plan(cfg):
    """(units, chunks, per_chunk, parts) of the weight gradient as fd_plan (sc_host_fdconv.h) cuts it"""
    dense = cfg["route"] == MFMA
    d = (1,) * (3 - len(cfg["dims"])) + tuple(cfg["dims"])
    tr, tc = (FDM_TR, FDM_TC) if dense else (FD_TR, FD_TC)
    units = cfg["batch"] * (1 if dense else d[0]) * (-(-d[1] // tr)) * (-(-d[2] // tc))
    jobs = cfg["c_out"] * (cfg["c_in"] // cfg["groups"]) * (cfg["k"] if len(cfg["dims"]) == 3 else 1)
    want = 64 if dense else (1 if jobs >= 1024 else min(1024 // jobs, 32))
    chunks = min(units, want)
    return units, chunks, -(-units // chunks), 4 * chunks if dense else chunks


def roundings(cfg):
    """N of (out, gx, gw): the fp32 roundings on the longest path to one element, counted in sc_kernels_fdconv.h.
    A folded weight carries fold = taps + 1 of them: taps - 1 additions of the centre tap's sum (k_fdconv_fold), its
    product with 1 / h, and the rounding of 1 / h to fp32 by the caller.
      out   fold + one fmaf per (input channel of the group, tap)                                     k_fdconv, fdm_conv
      gx    fold + one fmaf per (output channel of the group, tap); replicate / reflect add the pre-image sum of
            k_fdconv_unpad, (r + 1)^nd terms at a corner at the most
      gw    one fmaf per (batch entry, point) + the 8 levels of fd_block_sum (general route; the matrix-core route adds
            its four waves in the partial sum instead) + the partial sums of k_fdconv_wreduce + the subtraction, the
            product with 1 / h and the rounding of 1 / h
    Any order of summation stays below these, so they hold for both routes."""
    nd, r = len(cfg["dims"]), cfg["k"] // 2
    taps = cfg["k"] ** nd
    fold = taps + 1
    pts = int(np.prod(cfg["dims"]))
    unpad = (r + 1) ** nd if cfg["padding"] in ("replicate", "reflect") else 0
    return (fold + (cfg["c_in"] // cfg["groups"]) * taps,
            fold + (cfg["c_out"] // cfg["groups"]) * taps + unpad,
            cfg["batch"] * pts + 8 + wgrad_plan(cfg)[3] + 3)


def abs_bounds(cfg, x, w, g, grid_width):
    """((A_out, A_gx, A_gw), (N_out, N_gx, N_gw)): A is the layer on absolute values in float64 -- |x| and |g| with a
    kernel whose off-centre taps are |W| / |h| and whose centre tap is sum |W_offcentre| / |h| (the size of the terms of
    the cancelling fold as well); A_gw[t] = (A_G[t] + A_G[centre]) / |h| with A_G = sum |g| |xpad|, 0 at the centre."""
    nd, r, groups = len(cfg["dims"]), cfg["k"] // 2, cfg["groups"]
    conv = getattr(F, f"conv{nd}d")
    ah = abs(float(grid_width))
    x64 = x.detach().double().cpu().abs().requires_grad_(True)
    flat = w.detach().double().cpu().abs().reshape(*w.shape[:2], -1) / ah
    c = flat.shape[-1] // 2
    flat[..., c] = 0.0
    flat[..., c] = flat.sum(-1)
    ones = torch.ones_like(w, dtype=torch.float64).requires_grad_(True)   # d / d ones of sum |g| conv(|xpad|, ones) = A_G
    xp = F.pad(x64, [r, r] * nd, mode=PAD_MODE[cfg["padding"]])
    g64 = g.detach().double().cpu().abs()
    out = conv(xp, flat.reshape(w.shape), groups=groups)
    out.backward(g64, retain_graph=True)
    a_gx = x64.grad.clone()
    (a_g,) = torch.autograd.grad(conv(xp.detach(), ones, groups=groups), ones, g64)
    a_g = a_g.reshape(*w.shape[:2], -1)
    a_gw = (a_g + a_g[..., c:c + 1]) / ah
    a_gw[..., c] = 0.0
    return (out.detach().numpy(), a_gx.numpy(), a_gw.reshape(w.shape).numpy()), roundings(cfg)


def worst_ratio(got, want, bound, n):
    """max |got - want| / (gamma_n bound) over the elements; where bound == 0 the value must be exactly 0 (inf if not)"""
    got, want, bound = (np.asarray(t, np.float64) for t in (got, want, bound))
    err, lim = np.abs(got - want), gamma(n) * bound
    zero = bound == 0
    if (zero & (got != 0)).any() or not np.isfinite(got).all():
        return float("inf")
    return float((err[~zero] / lim[~zero]).max()) if (~zero).any() else 0.0


# ---- the verbatim reference, where it exists --------------------------------------------------------------------------
def _reference_file():
    from oracle import ref_verbatim
    return os.path.join(ref_verbatim.REFERENCE_ROOT, "neuralop", "layers", "differential_conv.py")


def reference_available():
    return os.path.isfile(_reference_file())


def load_reference_class():
    """the verbatim FiniteDifferenceConvolution, its file loaded by path: neuralop.layers as a package pulls in the
    discrete-continuous convolutions, which need torch_harmonics"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_verbatim_differential_conv", _reference_file())
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.FiniteDifferenceConvolution
