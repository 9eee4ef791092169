"""What the tests of the equidistant discrete-continuous convolutions share: a loader of the verbatim reference files
(by path, with a stand-in ``torch_harmonics`` in sys.modules while they load -- its filter_basis is the project's own
basis, its quadrature._precompute_grid raises), the case table of the recorder and the tests, and a float64 helper for
the convolution, its adjoint and their gradients.  torch on the host, no engine."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GENERAL, MFMA = 1, 2
NAME = "_verbatim_discrete_continuous_convolution"


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


# ---- cases: constructor arguments of the layer, batch, and what the issue expects of them ------------------------------
def _case(in_shape, out_shape, c_in=3, c_out=4, kernel_shape=(2, 4), batch=2, transposed=False, expect=None, **kw):
    ks = kernel_shape if isinstance(kernel_shape, int) else list(kernel_shape)
    return dict(kwargs=dict(in_channels=c_in, out_channels=c_out, in_shape=tuple(in_shape), out_shape=tuple(out_shape),
                            kernel_shape=ks, **kw),
                batch=batch, transposed=transposed, expect=expect or {})


# expect: attribute values the reference is known to give (psi_local_h x psi_local_w is the support of the local grid;
# the convolution kernel formed from the swapped, flipped buffer is psi_local_w tall and psi_local_h wide)
CASES = {
    "default": _case((16, 16), (16, 16), expect=dict(psi_local_h=3, psi_local_w=3, kernel_size=5)),
    "float_rounding_49": _case((49, 49), (49, 49), c_in=2, c_out=2, batch=1, expect=dict(psi_local_h=2, psi_local_w=2)),
    "rectangular_32x48": _case((32, 48), (32, 48), c_in=2, c_out=3, batch=1, expect=dict(psi_local_h=3, psi_local_w=4)),
    "stride2": _case((16, 16), (8, 8), expect=dict(psi_local_h=5, psi_local_w=5, scale_h=2, scale_w=2)),
    "strides_2x3": _case((32, 48), (16, 16), c_in=2, c_out=3, batch=1,
                         expect=dict(psi_local_h=5, psi_local_w=7, scale_h=2, scale_w=3)),
    "even_support_8": _case((16, 16), (16, 16), radius_cutoff=0.45, expect=dict(psi_local_h=8, psi_local_w=8)),
    "kernel_shape_3": _case((16, 16), (16, 16), kernel_shape=3, expect=dict(kernel_size=7)),
    "kernel_shape_3x4": _case((16, 16), (16, 16), kernel_shape=(3, 4), expect=dict(kernel_size=9)),
    "groups2": _case((16, 16), (16, 16), c_in=6, c_out=4, groups=2),
    "depthwise": _case((16, 16), (8, 8), c_in=4, c_out=4, groups=4),
    "no_bias": _case((16, 16), (16, 16), bias=False),
    "periodic": _case((16, 16), (16, 16), periodic=True),
    "transpose_stride2": _case((8, 8), (16, 16), transposed=True, expect=dict(scale_h=2, scale_w=2)),
    "transpose_strides_2x3": _case((16, 16), (32, 48), c_in=2, c_out=3, batch=1, transposed=True,
                                   expect=dict(scale_h=2, scale_w=3)),
    "transpose_scale1": _case((8, 8), (8, 8), transposed=True, expect=dict(psi_local_h=3, psi_local_w=3)),
    "transpose_grouped": _case((8, 8), (16, 16), c_in=4, c_out=6, groups=2, transposed=True),
}
ATTRS = ("kernel_shape", "kernel_size", "groups", "groupsize", "padding_mode", "domain_length", "psi_local_h",
         "psi_local_w", "scale_h", "scale_w", "q_weight")
NUMERIC_ATTRS = ("kernel_size", "groups", "groupsize", "psi_local_h", "psi_local_w", "scale_h", "scale_w", "q_weight")


def fp32_randn(shape, gen):
    return torch.randn(*shape, generator=gen, dtype=torch.float32)


def case_inputs(cfg, module, seed):
    """fp32 input, weight and bias (None without one) for `module` built from cfg"""
    g = torch.Generator().manual_seed(seed)
    kw = cfg["kwargs"]
    x = fp32_randn((cfg["batch"], kw["in_channels"], *kw["in_shape"]), g)
    w = fp32_randn(tuple(module.weight.shape), g) * float(1.0 / np.sqrt(module.groupsize))
    b = None if module.bias is None else fp32_randn((kw["out_channels"],), g)
    return x, w, b


def cotangent(shape, seed):
    return fp32_randn(tuple(shape), torch.Generator().manual_seed(seed + 100000))


# ---- float64 helper -----------------------------------------------------------------------------------------------------
def geometry(psi_local_h, psi_local_w, scale_h, scale_w, transposed):
    """(stride, padding, output_padding) of the reference's conv2d / conv_transpose2d call"""
    pad = ((psi_local_h + 1) // 2 - 1, (psi_local_w + 1) // 2 - 1)
    opad = (0, 0)
    if transposed:
        opad = (scale_h - (psi_local_h // 2 - pad[0]) - 1, scale_w - (psi_local_w // 2 - pad[1]) - 1)
    return (scale_h, scale_w), pad, opad


def disco(x, weight, bias, psi, q_weight, stride, padding, output_padding, groups, transposed):
    """the layer in the dtype of its inputs: psi = get_local_filter_matrix() (K, kh, kw)"""
    kernel = q_weight * torch.einsum("kxy,ogk->ogxy", psi, weight)
    if transposed:
        return F.conv_transpose2d(x, kernel, bias, stride=stride, padding=padding, output_padding=output_padding,
                                  groups=groups)
    return F.conv2d(x, kernel, bias, stride=stride, padding=padding, groups=groups)


def out_shape_of(x_shape, c_out, psi_shape, stride, padding, output_padding, transposed):
    (kh, kw), (h, w) = psi_shape[1:], x_shape[2:]
    if transposed:
        return (x_shape[0], c_out, (h - 1) * stride[0] - 2 * padding[0] + kh + output_padding[0],
                (w - 1) * stride[1] - 2 * padding[1] + kw + output_padding[1])
    return (x_shape[0], c_out, (h + 2 * padding[0] - kh) // stride[0] + 1, (w + 2 * padding[1] - kw) // stride[1] + 1)


def disco_with_grads(x, weight, bias, psi, g, q_weight, stride, padding, output_padding, groups, transposed):
    """(out, gx, gw, gbias) in float64 (gbias None without a bias) for fp32 or float64 host tensors"""
    x64 = x.detach().double().cpu().requires_grad_(True)
    w64 = weight.detach().double().cpu().requires_grad_(True)
    b64 = None if bias is None else bias.detach().double().cpu().requires_grad_(True)
    out = disco(x64, w64, b64, psi.detach().double().cpu(), q_weight, stride, padding, output_padding, groups,
                transposed)
    out.backward(g.detach().double().cpu())
    return out.detach(), x64.grad, w64.grad, None if b64 is None else b64.grad


# ---- free-standing descriptors through the C-ABI (the emulation and the GPU tier run the same runner and list) --------
def desc_case(in_shape, support, c_in=3, c_out=5, stride=(1, 1), padding=None, opad=(0, 0), groups=1, basis=4, batch=2,
              transposed=False, bias=True, route=GENERAL):
    padding = tuple((p + 1) // 2 - 1 for p in support) if padding is None else padding
    return dict(in_shape=in_shape, support=support, c_in=c_in, c_out=c_out, stride=stride, padding=padding, opad=opad,
                groups=groups, basis=basis, batch=batch, transposed=transposed, bias=bias, route=route)


DESC_CASES = {
    "3x3_one_past_a_tile_column": desc_case((5, 65), (3, 3)),
    "3x3_one_past_a_tile_row": desc_case((17, 6), (3, 3), batch=1),
    "5x5_stride2": desc_case((18, 21), (5, 5), stride=(2, 2)),
    "7x5_strides_3x4_pad_small": desc_case((20, 23), (7, 5), stride=(3, 4), padding=(1, 0), batch=1),
    "4x3_even_rectangular": desc_case((9, 10), (4, 3)),
    "2x2_pad0": desc_case((7, 7), (2, 2)),
    "15x15_cap": desc_case((17, 16), (15, 15), c_in=2, c_out=2, batch=1),
    "1x1": desc_case((4, 5), (1, 1)),
    "groups2_odd_channels": desc_case((6, 7), (3, 3), c_in=6, c_out=10, groups=2),
    "depthwise_one_row": desc_case((1, 9), (3, 3), c_in=5, c_out=5, groups=5),
    "no_bias_stride4": desc_case((16, 12), (5, 9), stride=(4, 4), bias=False, batch=1),
    "transpose_stride2": desc_case((5, 6), (5, 5), stride=(2, 2), opad=(1, 1), transposed=True),
    "transpose_strides_2x3_grouped": desc_case((4, 5), (7, 5), c_in=4, c_out=6, stride=(2, 3), opad=(1, 0), groups=2,
                                               transposed=True),
    "transpose_stride1_even": desc_case((6, 6), (4, 4), padding=(2, 2), transposed=True, batch=1),
    "transpose_past_a_tile": desc_case((9, 33), (3, 3), stride=(2, 2), opad=(1, 1), c_in=2, c_out=3, batch=1,
                                       transposed=True),
    "mfma_32_32": desc_case((5, 34), (3, 3), c_in=32, c_out=32, batch=1, route=MFMA),
    "mfma_64_32_no_bias": desc_case((4, 8), (3, 3), c_in=64, c_out=32, batch=1, bias=False, route=MFMA),
    "mfma_32_64_transposed": desc_case((4, 8), (3, 3), c_in=32, c_out=64, batch=2, transposed=True, route=MFMA),
}


def _for_output(out_shape, support, stride=(1, 1), padding=None, **kw):
    """a plain case with the smallest input that gives `out_shape`: in = (out - 1) stride + support - 2 padding"""
    padding = tuple((p + 1) // 2 - 1 for p in support) if padding is None else padding
    in_shape = tuple((o - 1) * s + k - 2 * p for o, s, k, p in zip(out_shape, stride, support, padding))
    return desc_case(in_shape, support, stride=stride, padding=padding, **kw)


# Kernel-edge cases: the tile, stride, chunk and route edges of sc_kernels_disco.h, run on the device by
# tests/test_gpu_disco_kernels.py; EMU_KERNEL_CASES names those the one-thread-per-lane emulation finishes in seconds.
# Groups are lettered as in that file's docstring.
def _kernel_cases():
    c = {}
    tr = {1: 16, 2: 8, 3: 4, 4: 4}
    for sh, sw in ((1, 1), (2, 2), (3, 3), (4, 4), (3, 4), (4, 3), (1, 4), (4, 1)):   # a: every row stride past its tile
        c[f"a_stride_{sh}x{sw}"] = _for_output((tr[sh] + 1, 65), (5, 5), stride=(sh, sw), padding=(2, 2))
    # b: the widest LDS tile (63 * 4 + 15 = 267 columns by 27 rows) and the tallest (30 rows), filled with data
    c["b_15x15_stride4_widest_tile"] = desc_case((20, 260), (15, 15), stride=(4, 4), c_in=2, c_out=2, batch=1)  # -> (5, 65)
    c["b_15x15_stride1_tallest_tile"] = _for_output((17, 65), (15, 15), padding=(7, 7), c_in=2, c_out=2, batch=1)
    for sup in ((4, 3), (1, 9)):                             # c: the padding extremes the host accepts
        for s in (1, 3):
            c[f"c_{sup[0]}x{sup[1]}_stride{s}_pad0"] = _for_output((5, 65), sup, stride=(s, s), padding=(0, 0))
            c[f"c_{sup[0]}x{sup[1]}_stride{s}_pad_support_less_1"] = _for_output(
                (5, 65), sup, stride=(s, s), padding=(sup[0] - 1, sup[1] - 1))
    for (sh, sw), pad in (((3, 4), (1, 0)), ((4, 3), (0, 2))):   # d: transposed, the first tile's floordiv arguments < 0
        for opad in ((0, 0), (sh - 1, sw - 1)):
            tag = f"d_transpose_{sh}x{sw}_opad{opad[0]}{opad[1]}"
            kw = dict(stride=(sh, sw), padding=pad, opad=opad, transposed=True)
            c[tag] = desc_case((6, 22), (7, 9), c_in=3, c_out=4, **kw)
            c[tag + "_groups2"] = desc_case((6, 22), (7, 9), c_in=4, c_out=6, groups=2, **kw)
    for n in (7, 8, 9):                                      # e: channels of a group around DC_OCB, both directions
        c[f"e_channels_{n}_groups1"] = desc_case((6, 7), (3, 3), c_in=n, c_out=n)
        c[f"e_channels_{n}_groups2"] = desc_case((6, 7), (3, 3), c_in=2 * n, c_out=2 * n, groups=2)
        c[f"e_channels_{n}_transposed"] = desc_case((6, 7), (3, 3), c_in=n, c_out=n, transposed=True, padding=(1, 1))
    c["e_depthwise9"] = desc_case((6, 7), (3, 3), c_in=9, c_out=9, groups=9)
    for pw in (1, 8, 9, 15):                                 # f: both reduction batches of k_disco_wgrad, with a stride
        for s in (1, 3):
            c[f"f_pw{pw}_stride{s}"] = _for_output((5, 7), (3, pw), stride=(s, s), c_in=2, c_out=3)
    c["f_one_chunk_33_31"] = desc_case((6, 7), (3, 3), c_in=33, c_out=31, batch=1)       # 3069 jobs >= 1024
    c["f_33_units_32_chunks"] = _for_output((41, 5), (3, 3), stride=(4, 1), c_in=2, c_out=2, batch=3)
    c["f_basis1"] = desc_case((6, 7), (3, 3), basis=1)
    c["f_basis40_nw_280"] = desc_case((6, 7), (3, 3), c_in=1, c_out=7, basis=40)         # 280 weight entries: two blocks
    for shape in ((3, 85), (16, 16), (1, 257)):              # bias gradient: 255, 256, 257 points to an image
        c[f"f_gbias_{shape[0] * shape[1]}_points"] = desc_case(shape, (3, 3), c_in=2, c_out=3, batch=3)
    for ci in (32, 64, 128):                                 # g: matrix cores, one past FDM_TR and FDM_TC
        for co in (32, 64, 128):
            for tp in (False, True):
                for bias in (True, False):
                    c[f"g_mfma_{ci}_{co}{'_transposed' if tp else ''}{'' if bias else '_no_bias'}"] = desc_case(
                        (5, 33), (3, 3), c_in=ci, c_out=co, batch=1, transposed=tp, bias=bias, route=MFMA)
    c["g_mfma_32_32_49x129_65_units"] = desc_case((49, 129), (3, 3), c_in=32, c_out=32, batch=1, route=MFMA)
    return c


KERNEL_CASES = _kernel_cases()
EMU_KERNEL_CASES = ("e_channels_9_groups1", "e_depthwise9", "f_basis1", "f_basis40_nw_280")


def weight_shape(cfg):
    if cfg["transposed"]:
        return (cfg["c_in"], cfg["c_out"] // cfg["groups"], cfg["basis"])
    return (cfg["c_out"], cfg["c_in"] // cfg["groups"], cfg["basis"])


def desc_inputs(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    x = fp32_randn((cfg["batch"], cfg["c_in"], *cfg["in_shape"]), g)
    w = fp32_randn(weight_shape(cfg), g) * 0.3
    psi = fp32_randn((cfg["basis"], *cfg["support"]), g)
    b = fp32_randn((cfg["c_out"],), g) if cfg["bias"] else None
    shape = out_shape_of(x.shape, cfg["c_out"], psi.shape, cfg["stride"], cfg["padding"], cfg["opad"],
                         cfg["transposed"])
    return x, w, psi, b, fp32_randn(shape, g)


Q = 0.0625


def desc_of(cfg, out_shape, **over):
    from neuraloperator_amd import _lib
    kw = dict(batch=cfg["batch"], c_in=cfg["c_in"], c_out=cfg["c_out"], in_shape=cfg["in_shape"], out_shape=out_shape,
              basis=cfg["basis"], support=cfg["support"], stride=cfg["stride"], padding=cfg["padding"],
              output_padding=cfg["opad"], groups=cfg["groups"], q_weight=Q, transposed=cfg["transposed"])
    kw.update(over)
    return _lib.ScEngineLib.disco_desc(**kw)


def run_descriptor(lib, cfg, x, w, psi, b, g, want=(True, True, True), device="cpu", stream=0):
    """sc_disco_forward + sc_disco_backward on tensors moved to `device`: (out, gx, gw, gbias) on the host"""
    x, w, psi, g = (t.to(device) for t in (x, w, psi, g))
    b = None if b is None else b.to(device)
    d = desc_of(cfg, g.shape[2:])
    nbytes, fbytes = lib.disco_workspace_bytes(d), lib.disco_forward_workspace_bytes(d)
    assert 0 < fbytes <= nbytes
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    y = torch.full(tuple(g.shape), float("nan"), device=device)
    lib.disco_forward(d, x.data_ptr(), w.data_ptr(), psi.data_ptr(), 0 if b is None else b.data_ptr(), y.data_ptr(),
                      ws.data_ptr(), fbytes, stream)         # its own, smaller size
    gx = torch.full_like(x, float("nan")) if want[0] else None
    gw = torch.full_like(w, float("nan")) if want[1] else None
    gb = torch.full((cfg["c_out"],), float("nan"), device=device) if want[2] else None
    ws.fill_(0xff)                                           # the backward call owes nothing to the forward call's workspace
    lib.disco_backward(d, x.data_ptr(), w.data_ptr(), psi.data_ptr(), g.data_ptr(), *(0 if t is None else t.data_ptr()
                                                                                        for t in (gx, gw, gb)),
                       ws.data_ptr(), nbytes, stream)
    return tuple(None if t is None else t.cpu() for t in (y, gx, gw, gb))


def desc_want(cfg, x, w, psi, b, g):
    out, gx, gw, gb = disco_with_grads(x, w, b, psi, g, Q, cfg["stride"], cfg["padding"], cfg["opad"], cfg["groups"],
                                       cfg["transposed"])
    if gb is None:                                           # the bias gradient does not need a bias
        gb = g.double().sum(dim=(0, 2, 3))
    return out, gx, gw, gb


# ---- per-element bound: |got - want| <= gamma_N A ----------------------------------------------------------------------
U = 2.0 ** -24                                               # unit round-off of fp32


def gamma(n):
    return n * U / (1.0 - n * U)


def worst_ratio(got, want, bound, n):
    """max |got - want| / (gamma_n bound) over the elements; where bound == 0 the value must be exactly 0 (inf if not)"""
    got, want, bound = (np.asarray(t, np.float64) for t in (got, want, bound))
    err, lim = np.abs(got - want), gamma(n) * bound
    zero = bound == 0
    if (zero & (got != 0)).any() or not np.isfinite(got).all():
        return float("inf")
    return float((err[~zero] / lim[~zero]).max()) if (~zero).any() else 0.0


def wgrad_plan(cfg, out_shape):
    """(units, chunks, per_chunk, parts) of the weight gradient as dc_plan (sc_host_disco.h) cuts it"""
    dense = cfg["route"] == MFMA
    hc, wc = cfg["in_shape"] if cfg["transposed"] else out_shape
    tr = {1: 16, 2: 8}.get(cfg["stride"][0], 4)
    tiles = (-(-hc // 4)) * (-(-wc // 32)) if dense else (-(-hc // tr)) * (-(-wc // 64))
    units = cfg["batch"] * tiles
    jobs = cfg["c_out"] * cfg["c_in"] // cfg["groups"] * cfg["support"][0]
    want = 64 if dense else (1 if jobs >= 1024 else min(1024 // jobs, 32))
    chunks = min(units, want)
    return units, chunks, -(-units // chunks), 4 * chunks if dense else chunks


def roundings(cfg, out_shape):
    """N of (out, gx, gw, gbias): the fp32 roundings on the longest path to one element, counted in sc_kernels_disco.h.
    A folded kernel entry carries fold = nk + 1 of them (k_disco_fold: nk fmaf and the product with q).
      out    fold + one fmaf per (input channel of the group, tap) + the bias          k_disco_conv / convT, fdm_conv
      gx     fold + one fmaf per (output channel of the group, tap)
      gw     one fmaf per (batch entry, coarse point) + the 8 levels of fd_block_sum + the partial sums (k_disco_psum;
             on the matrix cores one partial per wave) + one fmaf per tap and the product with q (k_disco_wreduce)
      gbias  a thread's chain over batch x ceil(points / 256) values + the 8 levels of fd_block_sum
    Any order of summation stays below these, so they hold for both routes and both forms."""
    taps, fold = cfg["support"][0] * cfg["support"][1], cfg["basis"] + 1
    hc, wc = cfg["in_shape"] if cfg["transposed"] else out_shape
    pts = out_shape[0] * out_shape[1]
    return (fold + (cfg["c_in"] // cfg["groups"]) * taps + 1,
            fold + (cfg["c_out"] // cfg["groups"]) * taps,
            cfg["batch"] * hc * wc + 8 + wgrad_plan(cfg, out_shape)[3] + taps + 1,
            cfg["batch"] * (-(-pts // 256)) + 8)


def abs_bounds(cfg, x, w, psi, b, g):
    """((A_out, A_gx, A_gw, A_gbias), (N ..)): A is the layer and its gradients in float64 on |x|, |w|, |psi|, |q|,
    |bias| with cotangent |g|"""
    ab = None if b is None else b.abs()
    out, gx, gw, gb = disco_with_grads(x.abs(), w.abs(), ab, psi.abs(), g.abs(), abs(Q), cfg["stride"], cfg["padding"],
                                       cfg["opad"], cfg["groups"], cfg["transposed"])
    if gb is None:
        gb = g.double().abs().sum(dim=(0, 2, 3))
    return (out, gx, gw, gb), roundings(cfg, tuple(g.shape[2:]))


# ---- the verbatim reference, where it exists --------------------------------------------------------------------------
def _reference_root():
    from oracle import ref_verbatim
    return os.path.join(ref_verbatim.REFERENCE_ROOT, "neuralop", "layers")


def reference_available():
    return os.path.isfile(os.path.join(_reference_root(), "discrete_continuous_convolution.py"))


def _standin_torch_harmonics():
    from neuraloperator_amd import filter_basis as own

    def refuse(*a, **k):
        raise NotImplementedError("torch_harmonics.quadrature is not on this machine: tensor grids only")

    def missing(name):
        def ctor(*a, **k):
            raise NotImplementedError(f"the {name} filter basis needs the torch_harmonics package")
        return ctor

    th = types.ModuleType("torch_harmonics")
    th.quadrature = types.ModuleType("torch_harmonics.quadrature")
    th.quadrature._precompute_grid = refuse
    th.filter_basis = types.ModuleType("torch_harmonics.filter_basis")
    th.filter_basis.PiecewiseLinearFilterBasis = own.PiecewiseLinearFilterBasis
    th.filter_basis.MorletFilterBasis = missing("morlet")
    th.filter_basis.ZernikeFilterBasis = missing("zernike")
    return th


def _load(modname, path):
    spec = importlib.util.spec_from_file_location(modname, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[modname] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference_module(modname=NAME, filename="discrete_continuous_convolution.py"):
    """a verbatim reference file loaded by path while the stand-in torch_harmonics is in sys.modules"""
    th = _standin_torch_harmonics()
    names = ("torch_harmonics", "torch_harmonics.quadrature", "torch_harmonics.filter_basis")
    saved = {n: sys.modules.get(n) for n in names}
    sys.modules.update({"torch_harmonics": th, "torch_harmonics.quadrature": th.quadrature,
                        "torch_harmonics.filter_basis": th.filter_basis})
    try:
        sys.modules.pop(modname, None)
        return _load(modname, os.path.join(_reference_root(), filename))
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m


def reference_class(transposed):
    mod = load_reference_module()
    return mod.EquidistantDiscreteContinuousConvTranspose2d if transposed else mod.EquidistantDiscreteContinuousConv2d


def own_class(transposed):
    import neuraloperator_amd as na
    return na.EquidistantDiscreteContinuousConvTranspose2d if transposed else na.EquidistantDiscreteContinuousConv2d


def run_module(cfg, rec, device):
    """the project's layer built from cfg with the record's weight and bias, forward + backward on the record's x and g:
    (module, out, gx, gw, gbias) as host numpy arrays (gbias None without a bias)"""
    m = own_class(cfg["transposed"])(**cfg["kwargs"])
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(rec["weight"]))
        if m.bias is not None:
            m.bias.copy_(torch.from_numpy(rec["bias"]))
    m = m.to(device)
    x = torch.from_numpy(rec["x"]).to(device).requires_grad_(True)
    assert m.on_engine(x)
    out = m(x)
    out.backward(torch.from_numpy(rec["g"]).to(device))
    gb = None if m.bias is None else m.bias.grad.cpu().numpy()
    return m, out.detach().cpu().numpy(), x.grad.cpu().numpy(), m.weight.grad.cpu().numpy(), gb


def load_reference_local_no_block():
    """the verbatim ``neuralop.layers.local_no_block`` module, imported with its siblings from where they lie while the
    stand-in torch_harmonics is in sys.modules"""
    import importlib
    from oracle import ref_verbatim
    ref_verbatim.load_reference()                      # package stubs, utils, tensorly / tltorch stand-ins
    name = "neuralop.layers.local_no_block"
    if name in sys.modules:
        return sys.modules[name]
    th = _standin_torch_harmonics()
    names = ("torch_harmonics", "torch_harmonics.quadrature", "torch_harmonics.filter_basis")
    saved = {n: sys.modules.get(n) for n in names}
    sys.modules.update({"torch_harmonics": th, "torch_harmonics.quadrature": th.quadrature,
                        "torch_harmonics.filter_basis": th.filter_basis})
    try:
        return importlib.import_module(name)
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m
