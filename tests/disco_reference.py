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
