"""TEST INFRASTRUCTURE ONLY: what the tests of ``neuraloperator_amd.FiniteDiff`` / ``LpLoss`` / ``H1Loss`` share.

  * a loader for the verbatim ``neuralop/losses/differentiation.py`` and ``data_losses.py`` from where the reference
    lies (``data_losses`` imports ``.differentiation`` relatively: both are loaded under the stub packages of
    ``fourier_diff_reference.load_reference_differentiation``);
  * the fixture cases shared by the recorder (tests/record_finite_diff.py) and the tests, with ``run_all`` /
    ``run_losses`` that call every method and take gradients for seeded cotangents;
  * a float64 dense-matrix restatement written from the formulas -- every operator is, along one axis, an N x N matrix
    with central-difference bands inside and third-order one-sided rows of four entries at the ends of a non-periodic
    axis -- that does not go through the engine.  No reference source is copied here."""
import importlib.util
import math
import os
import sys

import numpy as np
import torch

import fourier_diff_reference as fr
from oracle import ref_verbatim

GOLDEN = fr.GOLDEN
rel_l2 = fr.rel_l2
LEAD = (2, 3)
# name -> (grid, h per axis, periodic per axis)
CASES = {
    "finite_diff_1d_4_np": ((4,), (0.7,), (False,)),
    "finite_diff_1d_2_p": ((2,), (1.3,), (True,)),
    "finite_diff_1d_3_p": ((3,), (0.9,), (True,)),
    "finite_diff_2d_5x7_mixed": ((5, 7), (0.6, 1.4), (False, True)),
    "finite_diff_2d_8x6_p": ((8, 6), (1.1, 0.8), (True, True)),
    "finite_diff_3d_4x5x6_npx": ((4, 5, 6), (0.5, 1.2, 0.9), (False, True, True)),
    "finite_diff_3d_4x5x6_npy": ((4, 5, 6), (0.5, 1.2, 0.9), (True, False, True)),
    "finite_diff_3d_4x5x6_npz": ((4, 5, 6), (0.5, 1.2, 0.9), (True, True, False)),
    "finite_diff_3d_6x4x5_p": ((6, 4, 5), (1.5, 0.4, 0.8), (True, True, True)),
}
# name -> (operand shape, d, measure, the non-periodic variant's flags)
LOSS_CASES = {
    "sobolev_loss_1d": ((2, 3, 11), 1, 1.7, (False,)),
    "sobolev_loss_2d": ((2, 3, 6, 9), 2, [1.3, 0.6], (False, True)),
    "sobolev_loss_3d": ((2, 2, 4, 5, 6), 3, [0.9, 1.6, 0.7], (True, False, False)),
}
QUAD_LIST, QUAD_FLOAT = [0.37, 0.21, 0.5], 0.25


def reference_available():
    return fr.reference_available() and os.path.isfile(
        os.path.join(ref_verbatim.REFERENCE_ROOT, "neuralop", "losses", "data_losses.py"))


def load_reference_losses():
    """(differentiation module, data_losses module), verbatim, loaded from where they lie"""
    diff = fr.load_reference_differentiation()
    name = "neuralop.losses.data_losses"
    if name not in sys.modules:
        path = os.path.join(ref_verbatim.REFERENCE_ROOT, "neuralop", "losses", "data_losses.py")
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return diff, sys.modules[name]


# ------------------------------------------------------------------------------------------------ float64 helper
def dense_matrix(n, h, order, periodic):
    """(N, N) float64: central differences inside, one-sided third-order rows at the ends of a non-periodic axis"""
    m = np.zeros((n, n))
    for i in range(n):
        if periodic or 0 < i < n - 1:
            taps = ((-1, -1.0), (1, 1.0)) if order == 1 else ((-1, 1.0), (0, -2.0), (1, 1.0))
            for o, c in taps:
                m[i, (i + o) % n] += c / (2.0 * h if order == 1 else h * h)
        elif i == 0:
            row = (-11.0, 18.0, -9.0, 2.0) if order == 1 else (2.0, -5.0, 4.0, -1.0)
            m[0, :4] = np.array(row) / (6.0 * h if order == 1 else h * h)
        else:
            row = (-2.0, 9.0, -18.0, 11.0) if order == 1 else (-1.0, 4.0, -5.0, 2.0)
            m[n - 1, n - 4:] = np.array(row) / (6.0 * h if order == 1 else h * h)
    return m


def apply_matrix(m, u, axis):
    """the (N, N) matrix along `axis` (negative) of a float64 tensor, differentiable"""
    m = torch.as_tensor(m, dtype=torch.float64)
    return torch.movedim(torch.tensordot(m, u, dims=([1], [u.dim() + axis])), 0, axis)


class F64FiniteDiff:
    """the class's methods on dense float64 matrices (float64 whatever the input dtype)"""

    def __init__(self, dim, h=1.0, periodic=None):
        self.dim = dim
        self.h = (h,) * dim if isinstance(h, (int, float)) else tuple(h)
        self.periodic = (True,) * dim if periodic is None else tuple(periodic)

    def _d(self, u, d, order):
        u = u.double()
        return apply_matrix(dense_matrix(u.shape[d - self.dim], self.h[d], order, self.periodic[d]), u, d - self.dim)

    def dx(self, u, order=1):
        return self._d(u, 0, order)

    def dy(self, u, order=1):
        return self._d(u, 1, order)

    def dz(self, u, order=1):
        return self._d(u, 2, order)

    def laplacian(self, u):
        return sum(self._d(u, d, 2) for d in range(self.dim))

    def gradient(self, u):
        if self.dim == 1:
            return self._d(u, 0, 1)
        return torch.stack([self._d(u, d, 1) for d in range(self.dim)], dim=-self.dim - 1)

    def _comp(self, v, c):
        return v[(Ellipsis, c) + (slice(None),) * self.dim]

    def divergence(self, v):
        return sum(self._d(self._comp(v, d), d, 1) for d in range(self.dim))

    def curl(self, v):
        c, d = self._comp, self._d
        if self.dim == 2:
            return d(c(v, 1), 0, 1) - d(c(v, 0), 1, 1)
        return torch.stack([d(c(v, 2), 1, 1) - d(c(v, 1), 2, 1), d(c(v, 0), 2, 1) - d(c(v, 2), 0, 1),
                            d(c(v, 1), 0, 1) - d(c(v, 0), 1, 1)], dim=-4)


def _quad(x, d, measure, quadrature):
    if quadrature is None:
        measure = [measure] * d if isinstance(measure, float) else measure
        return [measure[-j] / x.shape[-j] for j in range(d, 0, -1)]
    return [quadrature] * d if isinstance(quadrature, float) else list(quadrature)


def f64_loss(x, y, d, kind, p=2, h1=False, relative=True, take_root=True, reduction="sum", measure=1.0,
             quadrature=None, eps=1e-8, periodic=None):
    """the loss from its formula in float64, differentiable: per line num = sum |e|^p (Lp) or sum e^2 + sum_j (D_j e)^2
    (H1), den the same of y; abs: (prod(q) num)^(1/p); rel: num^(1/p) / (den^(1/p) + eps)"""
    x, y = x.double(), y.double()
    q = _quad(x, d, measure, quadrature)
    dims = tuple(range(-d, 0))
    if h1:
        fd = F64FiniteDiff(d, q, periodic)
        terms = lambda t: [t] + [fd._d(t, j, 1) for j in range(d)]
        num = sum((a - b).square().sum(dim=dims) for a, b in zip(terms(x), terms(y)))
        den = sum(b.square().sum(dim=dims) for b in terms(y))
        p = 2
    else:
        num = (x - y).abs().pow(p).sum(dim=dims)
        den = y.abs().pow(p).sum(dim=dims)
    root = take_root and p != 1
    if relative:
        v = num.pow(1.0 / p) / (den.pow(1.0 / p) + eps) if root else num / (den + eps)
    else:
        v = math.prod(q) * num
        v = v.pow(1.0 / p) if root else v
    return v.sum() if reduction == "sum" else v.mean()


# ------------------------------------------------------------------------------------------------ shared drivers
def run_all(fd, u, v, gseed, dim):
    """Every method of a FiniteDiff-like object on u / v (requires_grad leaves) with ``u.grad`` / ``v.grad`` for fixed
    random cotangents; a dict name -> tensor.  Used on the verbatim class (recording), the engine class and the helper."""
    out = {"dx1": fd.dx(u), "dx2": fd.dx(u, order=2), "laplacian": fd.laplacian(u), "gradient": fd.gradient(u),
           "divergence": fd.divergence(v)}
    if dim >= 2:
        out.update({"dy1": fd.dy(u), "dy2": fd.dy(u, order=2), "curl": fd.curl(v)})
    if dim >= 3:
        out.update({"dz1": fd.dz(u), "dz2": fd.dz(u, order=2)})
    g = torch.Generator().manual_seed(gseed)
    cot = {k: torch.randn(t.shape, generator=g, dtype=torch.float64).to(device=t.device, dtype=t.dtype)
           for k, t in sorted(out.items())}
    scal = sum((out[k] * cot[k]).sum() for k in out if k not in ("divergence", "curl"))
    vec = sum((out[k] * cot[k]).sum() for k in ("divergence", "curl") if k in out)
    gu, = torch.autograd.grad(scal, u)
    gv, = torch.autograd.grad(vec, v)
    res = {k: t.detach() for k, t in out.items()}
    res["grad_u"], res["grad_v"] = gu, gv
    return res


def loss_configs(d):
    """every recorded call of a loss case: (key, class name, constructor kwargs, method, call kwargs)"""
    cfgs = []
    for red in ("sum", "mean"):
        for kind in ("abs", "rel"):
            for root in (True, False):
                for p in (1, 2, 3):
                    cfgs.append((f"lp{p}_{kind}_root{int(root)}_{red}", "LpLoss", dict(p=p, reduction=red), kind,
                                 dict(take_root=root)))
                for var in ("per", "np"):
                    cfgs.append((f"h1{var}_{kind}_root{int(root)}_{red}", "H1Loss", dict(reduction=red, variant=var),
                                 kind, dict(take_root=root)))
    for p in (1, 2, 3):
        cfgs.append((f"lp{p}_abs_quadlist", "LpLoss", dict(p=p), "abs", dict(quadrature=QUAD_LIST[:d])))
    cfgs.append(("lp2_abs_quadfloat", "LpLoss", dict(p=2), "abs", dict(quadrature=QUAD_FLOAT)))
    for var in ("per", "np"):
        cfgs.append((f"h1{var}_abs_quadlist", "H1Loss", dict(variant=var), "abs", dict(quadrature=QUAD_LIST[:d])))
        cfgs.append((f"h1{var}_rel_quadlist", "H1Loss", dict(variant=var), "rel", dict(quadrature=QUAD_LIST[:d])))
        cfgs.append((f"h1{var}_call_quadfloat", "H1Loss", dict(variant=var), "__call__", dict(quadrature=QUAD_FLOAT)))
    cfgs.append(("lp2_call", "LpLoss", dict(p=2), "__call__", {}))
    return cfgs


def make_loss(classes, cls, d, measure, np_flags, kw):
    kw = dict(kw)
    var = kw.pop("variant", None)
    if cls == "H1Loss":
        flags = np_flags if var == "np" else (True,) * d
        kw.update({"periodic_in_" + "xyz"[a]: flags[a] for a in range(d)})
    return classes[cls](d=d, measure=measure, **kw)


def run_losses(classes, x, y, name):
    """every configuration of a loss case on the classes {"LpLoss": .., "H1Loss": ..}: key -> value, key + ":grad" ->
    the gradient of value * (1.25 + its index / 16) by x"""
    _, d, measure, np_flags = LOSS_CASES[name]
    out = {}
    for i, (key, cls, ckw, method, kw) in enumerate(loss_configs(d)):
        loss = make_loss(classes, cls, d, measure, np_flags, ckw)
        val = getattr(loss, method)(x, y, **kw)
        gx, = torch.autograd.grad(val * (1.25 + i / 16.0), x)
        out[key], out[key + ":grad"] = val.detach(), gx
    return out


def f64_losses(x, y, name):
    """the same dict from the float64 helper"""
    _, d, measure, np_flags = LOSS_CASES[name]
    out = {}
    for i, (key, cls, ckw, method, kw) in enumerate(loss_configs(d)):
        h1 = cls == "H1Loss"
        per = (np_flags if ckw.get("variant") == "np" else (True,) * d) if h1 else None
        rel = method in ("rel", "__call__")
        root = True if method == "__call__" else kw.get("take_root", True)
        val = f64_loss(x, y, d, method, p=ckw.get("p", 2), h1=h1, relative=rel, take_root=root,
                       reduction=ckw.get("reduction", "sum"), measure=measure, quadrature=kw.get("quadrature"),
                       periodic=per)
        gx, = torch.autograd.grad(val * (1.25 + i / 16.0), x)
        out[key], out[key + ":grad"] = val.detach(), gx
    return out


# ---- free-standing descriptors of sc_kernels_stencil.h through the C-ABI -----------------------------------------------
# The emulation tier (tests/test_emu_stencil.py, CPU tensors) and the GPU tier (tests/test_gpu_stencil_kernels.py,
# device="cuda:0") run the same runners against the same float64 numpy evaluation of the kernels' own formulas.
from fdconv_reference import U, gamma, worst_ratio  # noqa: E402,F401  (fp32 unit round-off, gamma_N, max |err| / bound)

BAND_TR, BAND_TC, SOB_LP_UNIT = 32, 64, 1024           # tile of k_band_apply, points of one Lp pass (sc_kernels_stencil.h)


def fold(idx, n, per):
    return idx % n if per else np.clip(idx, 0, n - 1)


def random_tables(rng, dims, periodic, n_tab, zero_row=None):
    """[n_tab][n][7] per axis; on a clamped axis the taps that leave the line are zero, as the contract demands.
    zero_row = (axis, index): that row of every table of the axis is all zero (the skipped-tap branch of axis 0)."""
    tabs = []
    for a, (n, per, k) in enumerate(zip(dims, periodic, n_tab)):
        t = rng.standard_normal((k, n, 7))
        if not per:
            i = np.arange(n)[:, None] + np.arange(-3, 4)[None, :]
            t[:, (i < 0) | (i >= n)] = 0
        if zero_row is not None and zero_row[0] == a:
            t[:, zero_row[1]] = 0
        tabs.append(t.astype(np.float32))
    return tabs


def want_band(u, u2, tabs, periodic, terms, n_out, scale, absolute=False):
    """float64 y[g, t] = scale[g] sum_j coef_j sum_o T[i][o] s[.., i + o]; absolute: the same sum of the absolute
    values of its products (|u| + |u2| for the fused difference) -- the A of the per-element bound"""
    mag = np.abs if absolute else (lambda t: t)
    if absolute:
        s = np.abs(u.astype(np.float64)) + (0 if u2 is None else np.abs(u2.astype(np.float64)))
    else:
        s = u.astype(np.float64) - (0 if u2 is None else u2.astype(np.float64))
    dims = s.shape[2:]
    y = np.zeros((s.shape[0], n_out) + dims)
    for src, out, coef, axis, tab in terms:
        f = s[:, src]
        cf = mag(np.float64(np.float32(coef)))
        if axis < 0:
            y[:, out] += cf * f
            continue
        n = dims[axis]
        shp = [1] * (1 + len(dims))
        shp[1 + axis] = n
        for o in range(-3, 4):
            c = mag(tabs[axis][tab][:, o + 3].astype(np.float64)).reshape(shp)
            y[:, out] += cf * c * np.take(f, fold(np.arange(n) + o, n, periodic[axis]), axis=1 + axis)
    return y * mag(np.asarray(scale, np.float64)).reshape((-1,) + (1,) * (1 + len(dims)))


def band_roundings(terms, n_out, fused, scaled):
    """N of one output element of k_band_apply, counted in its source: the fused difference on the way into LDS (1), the
    product coef * t[k] of a tap (1), one fmaf per tap -- 7 per stencil term, 1 per identity term -- in the longest
    output, sc = scale * scale_mul and sc * acc (2)"""
    fmas = max([sum(7 if a >= 0 else 1 for _, o, _, a, _ in terms if o == t) for t in range(n_out)] + [1])
    return fmas + 1 + (1 if fused else 0) + (2 if scaled else 1)


def random_terms(rng, n_src, n_out, ndim, n_tab, n_terms, empty=None):
    outs = [o for o in range(n_out) if o != empty]
    terms = []
    for j in range(n_terms):
        out = outs[j] if j < len(outs) else outs[rng.integers(len(outs))]
        axis = int(rng.integers(-1, ndim)) if j else ndim - 1
        terms.append((int(rng.integers(n_src)), out, float(rng.standard_normal()), axis,
                      0 if axis < 0 else int(rng.integers(n_tab[axis]))))
    return tuple(terms)


def run_band(lib, u, u2, tabs, periodic, terms, n_out, out_major, scale=None, scale_mul=None, device="cpu", stream=0,
             gap=0, sentinel=float("nan")):
    """one sc_band_apply call on tensors moved to `device`: y (groups, n_out, *dims) on the host.  gap > 0: every output
    lies `gap` floats from the next one (group-major strides only); the gaps come back in the second result."""
    groups, n_src = u.shape[:2]
    dims = tuple(u.shape[2:])
    pts = int(np.prod(dims))
    on = lambda t: None if t is None else t.contiguous().to(device)
    u, u2, scale, scale_mul = on(u), on(u2), on(scale), on(scale_mul)
    tt = [on(torch.from_numpy(t)) for t in tabs]
    if gap:
        assert not out_major
        y = torch.full((groups, n_out, pts + gap), sentinel, device=device)
        gs, os_ = n_out * (pts + gap), pts + gap
    else:
        y = torch.full((n_out, groups, *dims) if out_major else (groups, n_out, *dims), sentinel, device=device)
        gs, os_ = (pts, groups * pts) if out_major else (n_out * pts, pts)
    lib.band_apply(u.data_ptr(), 0 if u2 is None else u2.data_ptr(), y.data_ptr(), dims=dims, periodic=periodic,
                   groups=groups, n_src=n_src, n_out=n_out, terms=terms, tabs=[t.data_ptr() for t in tt],
                   n_tab=[t.shape[0] for t in tt], y_group_stride=gs, y_out_stride=os_,
                   scale=0 if scale is None else scale.data_ptr(),
                   scale_mul=0 if scale_mul is None else scale_mul.data_ptr(), stream=stream)
    y = y.cpu()
    if gap:
        return y[:, :, :pts].reshape(groups, n_out, *dims), y[:, :, pts:]
    return y.transpose(0, 1) if out_major else y


def _band(dims, periodic, groups=2, n_src=1, n_out=2, n_terms=0, terms=None, empty=None, fused=False, scaled=False,
          out_major=False, zero_row=None, gap=0):
    return dict(dims=tuple(dims), periodic=tuple(periodic), groups=groups, n_src=n_src, n_out=n_out, n_terms=n_terms,
                terms=terms, empty=empty, fused=fused, scaled=scaled, out_major=out_major, zero_row=zero_row, gap=gap)


def _per_axis_terms(ndim, n_out):
    """one stencil term per axis (table 0 and, on the last axis, table 1 as well) and an identity term"""
    t = [(0, a % n_out, 0.5 + 0.25 * a, a, 0) for a in range(ndim)]
    return tuple(t + [(0, (ndim - 1) % n_out, -1.25, ndim - 1, 1), (0, 0, 0.75, -1, 0)])


def _band_cases():
    c = {}
    for d in ((31, 63), (32, 64), (33, 65), (1, 65), (33, 1)):          # 1a: one short of, at and one past the tile
        name = "x".join(map(str, d))
        c[f"a_{name}_periodic"] = _band(d, (True, True), terms=_per_axis_terms(2, 2))
        clamp = tuple(n < 4 for n in d)
        c[f"a_{name}_clamped"] = _band(d, clamp, terms=_per_axis_terms(2, 2), fused=True)
    for d in ((1, 5, 6), (2, 5, 6), (3, 5, 6), (5, 1, 6), (5, 2, 6), (5, 3, 6), (5, 6, 1), (5, 6, 2), (5, 6, 3),
              (1, 1, 1)):                                               # 1b: the taps alias, on each internal axis
        c["b_" + "x".join(map(str, d)) + "_periodic"] = _band(d, (True,) * 3, n_out=3, terms=_per_axis_terms(3, 3))
    for d, per in (((4, 5, 6), (False, True, True)), ((5, 4, 6), (True, False, True)), ((5, 6, 4), (True, True, False)),
                   ((4, 4, 4), (False,) * 3)):                          # the smallest clamped extent
        c["b_" + "x".join(map(str, d)) + "_clamped4"] = _band(d, per, n_out=3, terms=_per_axis_terms(3, 3))
    for per0 in (False, True):                                          # 1c: axis-0 taps read from global memory
        tag = "periodic" if per0 else "clamped"
        c[f"c_7x33x65_axis0_{tag}"] = _band((7, 33, 65), (per0, True, False), terms=_per_axis_terms(3, 2))
        c[f"c_7x33x65_axis0_{tag}_zero_row"] = _band((7, 33, 65), (per0, True, False), terms=_per_axis_terms(3, 2),
                                                     zero_row=(0, 3))
        c[f"c_7x33x65_axis0_{tag}_fused"] = _band((7, 33, 65), (per0, True, False), terms=_per_axis_terms(3, 2),
                                                  fused=True)
    ident = tuple((s, o, 0.5 + s - o, -1, 0) for s in range(3) for o in range(3))
    c["d_twelve_slots"] = _band((5, 67), (True, False), groups=3, n_src=3, n_out=3,
                                terms=ident + ((0, 0, 1.5, 0, 0), (1, 1, -0.5, 1, 1), (2, 2, 2.0, 1, 0)))
    c["d_termless_output"] = _band((5, 67), (True, False), groups=3, n_src=2, n_out=3, n_terms=5, empty=1)
    c["d_scale_and_scale_mul"] = _band((5, 67), (True, False), groups=3, n_src=2, n_out=2, n_terms=5, scaled=True)
    c["d_out_major"] = _band((5, 67), (True, False), groups=3, n_src=2, n_out=3, n_terms=6, out_major=True, scaled=True)
    c["d_gaps_behind_every_output"] = _band((5, 67), (True, False), groups=3, n_src=1, n_out=2, n_terms=4, gap=3)
    c["e_4099_groups_3x5"] = _band((3, 5), (True, True), groups=4099, terms=_per_axis_terms(2, 2), scaled=True)
    return c


BAND_KERNEL_CASES = _band_cases()
# those the one-thread-per-lane emulation finishes in well under a second each
EMU_BAND_KERNEL_CASES = ("a_33x65_periodic", "a_33x1_clamped", "b_1x5x6_periodic", "b_2x5x6_periodic", "b_3x5x6_periodic",
                         "b_5x1x6_periodic", "b_5x2x6_periodic", "b_5x3x6_periodic", "b_1x1x1_periodic",
                         "b_4x4x4_clamped4", "d_twelve_slots", "d_gaps_behind_every_output")


def band_case_inputs(cfg, seed):
    """(u, u2, tabs, terms, scale, scale_mul) of a band case: host tensors / numpy tables"""
    rng = np.random.default_rng(seed)
    nd = len(cfg["dims"])
    n_tab = (2,) * nd
    tabs = random_tables(rng, cfg["dims"], cfg["periodic"], n_tab, cfg["zero_row"])
    terms = cfg["terms"] or random_terms(rng, cfg["n_src"], cfg["n_out"], nd, n_tab, cfg["n_terms"], cfg["empty"])
    shape = (cfg["groups"], cfg["n_src"]) + cfg["dims"]
    u = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    u2 = torch.from_numpy(rng.standard_normal(shape).astype(np.float32)) if cfg["fused"] else None
    scale = torch.from_numpy(rng.standard_normal(cfg["groups"]).astype(np.float32)) if cfg["scaled"] else None
    mul = torch.tensor([1.5]) if cfg["scaled"] else None
    return u, u2, tabs, terms, scale, mul


def run_band_case(lib, cfg, inputs, device="cpu", stream=0):
    u, u2, tabs, terms, scale, mul = inputs
    return run_band(lib, u, u2, tabs, cfg["periodic"], terms, cfg["n_out"], cfg["out_major"], scale, mul, device, stream,
                    gap=cfg["gap"], sentinel=7.0 if cfg["gap"] else float("nan"))


def band_expect(cfg, inputs):
    """(want, A, N): the float64 result, the sum of the absolute values of its products and the roundings"""
    u, u2, tabs, terms, scale, mul = inputs
    sc = np.ones(cfg["groups"]) if scale is None else scale.numpy().astype(np.float64) * float(mul)
    args = (u.numpy(), None if u2 is None else u2.numpy(), tabs, cfg["periodic"], terms, cfg["n_out"], sc)
    return want_band(*args), want_band(*args, absolute=True), band_roundings(terms, cfg["n_out"], cfg["fused"],
                                                                           cfg["scaled"])


# ---- the two data losses: k_sobolev_partial, k_loss_finish, k_lp_grad --------------------------------------------------
def want_sums(x, y, d, h1, p, tabs, periodic, absolute=False):
    """float64 (num, den) per line: sum |e|^p (Lp) or sum e^2 + sum_j (D_j e)^2 (H1), den the same of y.  absolute (H1):
    every stencil as the sum of the absolute values of its products -- the A of the bound (for Lp the terms are
    non-negative and A is the sum itself)"""
    x, y = x.astype(np.float64), y.astype(np.float64)
    dims = x.shape[1:]
    ax = tuple(range(1, 1 + d))
    mag = np.abs if absolute else (lambda t: t)

    def terms(f):
        out = [f]
        for a in range(d if h1 else 0):
            n = dims[a]
            shp = [1] * (1 + d)
            shp[1 + a] = n
            out.append(sum(mag(tabs[a][0][:, o + 3].astype(np.float64)).reshape(shp) *
                           np.take(mag(f), fold(np.arange(n) + o, n, periodic[a]), axis=1 + a) for o in range(-3, 4)))
        return out
    num = sum((np.abs(t) ** p).sum(axis=ax) for t in terms(x - y))
    den = sum((np.abs(t) ** p).sum(axis=ax) for t in terms(y))
    return num, den


def sob_plan(dims, h1, lines, chunks, cu_count=None):
    """(units, chunks, per_chunk in units) as sob_plan (sc_engine.cpp) cuts a line; chunks = 0 needs the CU count"""
    d = (1,) * (3 - len(dims)) + tuple(dims)
    pts = int(np.prod(d))
    units = d[0] * (-(-d[1] // BAND_TR)) * (-(-d[2] // BAND_TC)) if h1 else -(-pts // SOB_LP_UNIT)
    want = chunks if chunks else -(-4 * cu_count // max(lines, 1))
    want = max(1, min(want, units))
    per = -(-units // want)
    return units, -(-units // per), per


def finish_plan(lines, chunks):
    """(sub, passes, chunk terms per thread) of k_loss_finish"""
    sub = 1
    while sub < 256 and sub < chunks:
        sub <<= 1
    return sub, -(-lines // (256 // sub)), -(-chunks // sub)


def sums_roundings(h1, p, d, per_chunk):
    """N of one (line, chunk) partial sum of k_sobolev_partial, counted in its source.
    Lp: e = x - y (1) enters |e|^p p times and sob_powi multiplies p - 1 times: 2 p - 1; a pass adds four powers and the
    running sum: 4 per pass of SOB_LP_UNIT points; the LDS tree of sob_block_sum2: 8.
    H1: D e is 7 fmaf of rounded differences (1 + 7), squared: 2 * 8, its fmaf into the row sum 1; e * e and one fmaf
    per axis: 1 + d - 1 more; num += sn once per row, 8 rows per tile and thread; the tree: 8."""
    if h1:
        return 16 + 1 + d + BAND_TR // 4 * per_chunk + 8
    return 2 * p - 1 + 4 * per_chunk + 8


def finish_roundings(lines, chunks):
    """(chunk sum, value, loss): roundings k_loss_finish adds -- the strided chunk sum of a thread and its LDS tree;
    on the longest branch (relative, root) 1 / p, two roots, eps as fp32, + eps, the division, val * ip, / num, the
    reduction factor as fp32 and its product: 10; the sum of the lines (256 threads stride the lines, then 8 tree
    levels) and the factor"""
    sub, _, per_thread = finish_plan(lines, chunks)
    return per_thread + sub.bit_length() - 1, 10, -(-lines // 256) + 8 + 2


def loss_formulas(num, den, p, relative, root, mean, konst, eps, lines):
    """float64 (v, dv times the reduction factor, loss) of the finish kernel's formula from per-line sums"""
    r = root and p != 1
    with np.errstate(divide="ignore", invalid="ignore"):
        if relative:
            v = num ** (1 / p) / (den ** (1 / p) + eps) if r else num / (den + eps)
            dv = v / (p * num) if r else 1 / (den + eps)
        else:
            v = (konst * num) ** (1 / p) if r else konst * num
            dv = v / (p * num) if r else np.full(lines, konst)
    f = 1 / lines if mean else 1.0
    return v, dv * f, f * v.sum()


def _sums(dims, lines=1, h1=False, p=2, relative=True, root=True, mean=False, chunks=0, periodic=None, offset=None,
          same_line=None, zero_line=None):
    return dict(dims=tuple(dims), lines=lines, h1=h1, p=p, relative=relative, root=root, mean=mean, chunks=chunks,
                periodic=tuple(periodic) if periodic else (True,) * len(dims), offset=offset, same_line=same_line,
                zero_line=zero_line)


def _sums_cases():
    c = {}
    for pts, tag in ((300 * 1024, "vec"), (300 * 1024 + 7, "scalar")):          # 2a: chunk plans of one line
        for ch in (1, 5, 256, 257, 300, 0):
            c[f"a_lp_{tag}_chunks{ch}"] = _sums((pts,), chunks=ch, p=2, mean=ch % 2 == 1)
    for ch in (7, 299, 300):
        c[f"a_h1_640x960_chunks{ch}"] = _sums((640, 960), h1=True, chunks=ch, periodic=(True, False))
    c["b_lines257_chunks1"] = _sums((6, 7), lines=257, chunks=1, mean=True)      # 2b: passes of the finish kernel
    c["b_lines300_chunks1"] = _sums((6, 7), lines=300, chunks=1)
    c["b_lines300_chunks3"] = _sums((3000,), lines=300, chunks=3, mean=True, p=1)
    c["b_lines65_chunks5"] = _sums((5000,), lines=65, chunks=5, relative=False)
    c["b_h1_lines300_chunks3"] = _sums((3, 5, 6), lines=300, h1=True, chunks=3, periodic=(True, True, False))
    for n in (1, 2, 3, 4, 1023, 1024, 1025, 4100):                               # 2c: access width
        c[f"c_points{n}"] = _sums((n,), lines=3, p=3, chunks=2)
    for n in (1024, 4100):
        for which in ("x", "y", "gx"):
            c[f"c_points{n}_{which}_off_by_one_float"] = _sums((n,), lines=3, p=2, chunks=2, offset=which)
    for p in (1, 2, 3, 6):                                                       # 2d: every configuration once
        for rel in (True, False):
            for root in (True, False):
                for mean in (True, False):
                    c[f"d_lp{p}_{'rel' if rel else 'abs'}_root{int(root)}_{'mean' if mean else 'sum'}"] = \
                        _sums((5, 413), lines=5, p=p, relative=rel, root=root, mean=mean, chunks=2)
    # a clamped axis needs 4 points (sc_band_apply and sc_sobolev_sums refuse fewer): axis 0 is clamped at extent 4 and
    # periodic at extent 3, where axis 1 is the clamped one
    for dims, per in (((33, 65), (True, False)), ((4, 33, 65), (False, True, True)), ((3, 33, 65), (True, False, True))):
        for rel in (True, False):
            for root in (True, False):
                for mean in (True, False):
                    name = "x".join(map(str, dims))
                    c[f"d_h1_{name}_{'rel' if rel else 'abs'}_root{int(root)}_{'mean' if mean else 'sum'}"] = \
                        _sums(dims, lines=3, h1=True, relative=rel, root=root, mean=mean, chunks=2, periodic=per)
    for p in (1, 2, 3):                                                          # 2e: degenerate lines among ordinary ones
        for root in (True, False):
            c[f"e_lp{p}_root{int(root)}_degenerate_lines"] = _sums((1030,), lines=5, p=p, root=root, chunks=2,
                                                                    same_line=1, zero_line=3)
    for root in (True, False):
        c[f"e_h1_root{int(root)}_degenerate_lines"] = _sums((9, 70), lines=5, h1=True, root=root, chunks=2,
                                                             periodic=(False, True), same_line=1, zero_line=3)
    return c


SUMS_KERNEL_CASES = _sums_cases()
EMU_SUMS_KERNEL_CASES = ("a_lp_vec_chunks300",
                         "c_points1", "c_points3", "c_points1025", "c_points1024_gx_off_by_one_float",
                         "c_points4100_x_off_by_one_float", "d_lp6_rel_root1_mean", "d_lp3_abs_root0_sum",
                         "e_lp1_root1_degenerate_lines", "e_lp2_root1_degenerate_lines", "e_lp3_root0_degenerate_lines",
                         "e_h1_root1_degenerate_lines")
KONST, EPS, GOUT = 0.37, 1e-3, 0.75


def sums_case_inputs(cfg, seed):
    """(x, y, tabs): |x - y| <= 1 (so |e|^6 stays in range); the degenerate lines: x = y exactly, y = 0"""
    rng = np.random.default_rng(seed)
    shape = (cfg["lines"],) + cfg["dims"]
    y = rng.uniform(-0.5, 0.5, shape).astype(np.float32)
    x = (y + rng.uniform(-0.5, 0.5, shape).astype(np.float32)).astype(np.float32)
    if cfg["same_line"] is not None:
        x[cfg["same_line"]] = y[cfg["same_line"]]
    if cfg["zero_line"] is not None:
        y[cfg["zero_line"]] = 0
    tabs = random_tables(rng, cfg["dims"], cfg["periodic"], (2,) * len(cfg["dims"])) if cfg["h1"] else None
    if tabs is not None:
        tabs = [t * np.float32(0.25) for t in tabs]
    return torch.from_numpy(x), torch.from_numpy(y), tabs


def _placed(t, device, off):
    """t on `device`, `off` floats into a fresh allocation (torch's allocations are at least 16-byte aligned)"""
    store = torch.empty(t.numel() + 4, dtype=t.dtype, device=device)
    assert store.data_ptr() % 16 == 0
    v = store[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def run_sums_case(lib, cfg, inputs, device="cpu", stream=0):
    """sc_sobolev_sums (and sc_lp_grad for Lp, sc_band_apply with the per-line scale for H1) of a case: a dict of host
    tensors -- ws (lines, chunks, 2), v, dv, loss, gx (Lp) -- and the chunk count read back from the workspace size"""
    x, y, tabs = inputs
    lines, dims = cfg["lines"], cfg["dims"]
    off = {k: int(cfg["offset"] == k) for k in ("x", "y", "gx")}
    xd, yd = _placed(x, device, off["x"]), _placed(y, device, off["y"])
    tt = None if tabs is None else [torch.from_numpy(t).contiguous().to(device) for t in tabs]
    desc = lib.sobolev_desc(dims=dims, periodic=cfg["periodic"], lines=lines, h1=cfg["h1"], p=cfg["p"],
                            relative=cfg["relative"], take_root=cfg["root"], reduce_mean=cfg["mean"], konst=KONST, eps=EPS,
                            tabs=None if tt is None else [t.data_ptr() for t in tt], chunks=cfg["chunks"])
    nbytes = lib.sobolev_workspace_bytes(desc)
    assert nbytes > 0 and nbytes % (8 * lines) == 0
    n_chunks = nbytes // (8 * lines)
    ws = torch.full((nbytes // 4,), float("nan"), device=device)
    v, dv = torch.full((lines,), float("nan"), device=device), torch.full((lines,), float("nan"), device=device)
    loss = torch.full((1,), float("nan"), device=device)
    lib.sobolev_sums(desc, xd.data_ptr(), yd.data_ptr(), ws.data_ptr(), nbytes, v.data_ptr(), dv.data_ptr(),
                     loss.data_ptr(), stream)
    out = dict(n_chunks=n_chunks)
    if not cfg["h1"]:
        gout = torch.tensor([GOUT], device=device)
        gx = _placed(torch.full_like(x, float("nan")), device, off["gx"])
        lib.lp_grad(desc, xd.data_ptr(), yd.data_ptr(), dv.data_ptr(), gout.data_ptr(), gx.data_ptr(), stream)
        out["gx"] = gx.cpu()
    out.update(ws=ws.cpu().reshape(lines, n_chunks, 2), v=v.cpu(), dv=dv.cpu(), loss=loss.cpu())
    return out


def limit_ratio(got, want, lim):
    """max |got - want| / lim over the elements where `want` is finite; inf if `got` is finite anywhere else than
    `want`, or differs from it where lim is 0 (an exact value)"""
    got, want, lim = (np.atleast_1d(np.asarray(t, np.float64)) for t in (got, want, lim))
    lim = np.broadcast_to(lim, want.shape)
    ok = np.isfinite(want)
    if (np.isfinite(got) != ok).any():
        return float("inf")
    err = np.abs(got[ok] - want[ok])
    exact = lim[ok] == 0
    if (err[exact] != 0).any():
        return float("inf")
    return float((err[~exact] / lim[ok][~exact]).max()) if (~exact).any() else 0.0


def _finite_rel_l2(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ok = np.isfinite(want)
    return rel_l2(got[ok], want[ok]) if ok.any() else 0.0


def check_band_case(name, cfg, inputs, got):
    """the two bars of a band case (and its untouched gaps, its zero output); prints and returns (rel-L2, worst ratio)"""
    gaps = None
    if cfg["gap"]:
        got, gaps = got
    want, A, n = band_expect(cfg, inputs)
    assert not torch.isnan(got).any()                                    # every addressed element is overwritten
    rel, ratio = rel_l2(got.numpy(), want), worst_ratio(got.numpy(), want, A, n)
    print(f"{name} rel_l2 {rel:.1e} worst |err| / (gamma_N A) {ratio:.3f} (N={n})")
    assert rel <= 1e-5 and ratio <= 1.0, (name, rel, ratio)
    if cfg["empty"] is not None:
        assert torch.all(got[:, cfg["empty"]] == 0)
    if gaps is not None:
        assert torch.all(gaps == 7.0) and not torch.any(got == 7.0)
    return rel, ratio


def check_sums_case(name, cfg, inputs, got, lib, device="cpu", stream=0):
    """the bars of a loss case: partial sums, v, dv, the loss, the Lp gradient (H1, degenerate lines: the backward
    through sc_band_apply with the lines' scale); prints and returns the worst ratio"""
    x, y, tabs = inputs
    lines, dims, p, h1 = cfg["lines"], cfg["dims"], cfg["p"], cfg["h1"]
    d, n_chunks = len(dims), got["n_chunks"]
    num, den = want_sums(x.numpy(), y.numpy(), d, h1, p, tabs, cfg["periodic"])
    a_num, a_den = want_sums(x.numpy(), y.numpy(), d, h1, p, tabs, cfg["periodic"], absolute=True) if h1 else (num, den)
    units = sob_plan(dims, h1, lines, 1)[0]
    per = sob_plan(dims, h1, lines, cfg["chunks"])[2] if cfg["chunks"] else \
        (units if n_chunks == 1 else -(-units // (n_chunks - 1)))           # the default plan: an upper bound
    n1 = sums_roundings(h1, p, d, per)
    part = got["ws"].double().sum(dim=1).numpy()
    ratios = {"num": worst_ratio(part[:, 0], num, a_num, n1), "den": worst_ratio(part[:, 1], den, a_den, n1)}
    rels = {"num": rel_l2(part[:, 0], num), "den": rel_l2(part[:, 1], den)}
    nc, nf, nl = finish_roundings(lines, n_chunks)
    with np.errstate(divide="ignore", invalid="ignore"):
        rn = np.where(num > 0, gamma(n1 + nc) * a_num / num, 0.0)
        rd = np.where(den > 0, gamma(n1 + nc) * a_den / den, 0.0) if cfg["relative"] else np.zeros(lines)
    want_v, want_dv, want_loss = loss_formulas(num, den, p, cfg["relative"], cfg["root"], cfg["mean"], KONST, EPS, lines)
    v, dv, loss = got["v"].numpy(), got["dv"].numpy(), float(got["loss"])
    rels.update(v=_finite_rel_l2(v, want_v), dv=_finite_rel_l2(dv, want_dv),
                loss=abs(loss - want_loss) / abs(want_loss))
    powf = cfg["root"] and p > 2                                            # no stated error of powf: 1e-5 only
    if not powf:
        rv = rn + rd + gamma(nf)
        ratios["v"] = limit_ratio(v, want_v, rv * np.abs(want_v))
        ratios["dv"] = limit_ratio(dv, want_dv, (rv + rn) * np.abs(want_dv))
        ratios["loss"] = limit_ratio(loss, want_loss, (rv.max() + gamma(nl)) * abs(want_loss))
    else:
        assert np.array_equal(np.isfinite(dv), np.isfinite(want_dv)) and np.isfinite(v).all()
    if cfg["same_line"] is not None:
        assert v[cfg["same_line"]] == 0.0 and part[cfg["same_line"], 0] == 0.0
    e = x.numpy().astype(np.float64) - y.numpy().astype(np.float64)
    shp = (-1,) + (1,) * d
    if not h1:
        with np.errstate(invalid="ignore"):
            shape_g = GOUT * p * np.abs(e) ** (p - 1) * np.sign(e)
            own = dv.astype(np.float64).reshape(shp) * shape_g           # the kernel's formula on the dv it was given
            pure = want_dv.reshape(shp) * shape_g
        gx = got["gx"].numpy()
        ratios["gx"] = limit_ratio(gx, own, gamma(2 * p) * np.abs(own))
        rels["gx"] = _finite_rel_l2(gx, pure)
        assert np.array_equal(np.isfinite(gx), np.isfinite(pure))
    elif cfg["same_line"] is not None:
        terms = ((0, 0, 2.0, -1, 0),) + tuple((0, 0, 2.0, a, 1) for a in range(d))
        gout = torch.tensor([GOUT])
        gx = run_band(lib, x[:, None], y[:, None], tabs, cfg["periodic"], terms, 1, False, got["dv"], gout, device,
                      stream, sentinel=7.0)
        with np.errstate(invalid="ignore"):
            args = (x[:, None].numpy(), y[:, None].numpy(), tabs, cfg["periodic"], terms, 1)
            own = want_band(*args, dv.astype(np.float64) * GOUT)
            pure = want_band(*args, want_dv * GOUT)
            lim = gamma(band_roundings(terms, 1, True, True)) * want_band(*args, np.abs(dv.astype(np.float64)) * GOUT,
                                                                           absolute=True)
        ratios["gx_band"] = limit_ratio(gx.numpy(), own, lim)
        rels["gx_band"] = _finite_rel_l2(gx.numpy(), pure)
        assert np.array_equal(np.isfinite(gx.numpy()), np.isfinite(pure))
    print(f"{name} chunks {n_chunks} rel_l2 " + " ".join(f"{k}={r:.1e}" for k, r in rels.items()) +
          " worst |err| / bound " + " ".join(f"{k}={r:.3f}" for k, r in ratios.items()) +
          (" (powf: v, dv, loss at 1e-5 only)" if powf else ""))
    assert all(r <= 1e-5 for r in rels.values()), (name, rels)
    assert all(r <= 1.0 for r in ratios.values()), (name, ratios)
    return max(ratios.values())


def refused_stencil_arguments(lib, device="cpu"):
    """every refused sc_band_apply / sc_sobolev_sums / sc_lp_grad argument returns its error and launches nothing"""
    import pytest
    from neuraloperator_amd import _lib
    rng = np.random.default_rng(1)
    dims, periodic = (4, 6), (False, True)
    tabs = [torch.from_numpy(t).to(device) for t in random_tables(rng, dims, periodic, (2, 2))]
    u, y = torch.zeros(2, 2, 4, 6, device=device), torch.zeros(2, 2, 4, 6, device=device)
    ok = dict(dims=dims, periodic=periodic, groups=2, n_src=2, n_out=2, terms=((0, 0, 1.0, 0, 0), (1, 1, 1.0, -1, 0)),
              tabs=[t.data_ptr() for t in tabs], n_tab=(2, 2), y_group_stride=48, y_out_stride=24)
    lib.band_apply(u.data_ptr(), 0, y.data_ptr(), **ok)
    bad = [dict(dims=(4, 6, 2, 2)), dict(dims=(3, 6)), dict(dims=(4, 0)), dict(n_src=4), dict(n_src=0), dict(n_out=0),
           dict(n_out=4), dict(groups=-1), dict(terms=((2, 0, 1.0, 0, 0),)), dict(terms=((0, 2, 1.0, 0, 0),)),
           dict(terms=((0, 0, 1.0, 2, 0),)), dict(terms=((0, 0, 1.0, 0, 2),)), dict(terms=((0, 0, 1.0, 0, 0),) * 13),
           dict(terms=((0, 0, 1.0, 0, 0),) * 12), dict(y_out_stride=-1), dict(tabs=[0, 0])]
    for change in bad:
        with pytest.raises(_lib.EngineError):
            lib.band_apply(u.data_ptr(), 0, y.data_ptr(), **{**ok, **change})
    with pytest.raises(_lib.EngineError):
        lib.band_apply(0, 0, y.data_ptr(), **ok)
    with pytest.raises(_lib.EngineError):
        lib.band_apply(u.data_ptr(), 0, 0, **ok)
    lib.band_apply(0, 0, 0, **{**ok, "groups": 0})                        # no groups: nothing to do
    good = dict(dims=dims, periodic=periodic, lines=2, h1=True, relative=False, tabs=[t.data_ptr() for t in tabs])
    x = torch.zeros(2, 4, 6, device=device)
    v, dv, ws = torch.zeros(2, device=device), torch.zeros(2, device=device), torch.zeros(64, device=device)
    loss = torch.full((1,), 5.0, device=device)
    args = lambda: (x.data_ptr(), x.data_ptr(), ws.data_ptr(), 256, v.data_ptr(), dv.data_ptr(), loss.data_ptr())
    lib.sobolev_sums(lib.sobolev_desc(**good), *args())
    assert float(loss) == 0.0
    loss.fill_(5.0)
    for change in [dict(dims=(3, 6)), dict(p=0, h1=False), dict(p=3), dict(lines=-1), dict(tabs=[0, 0]),
                   dict(dims=(2, 6)), dict(chunks=-1)]:
        desc = lib.sobolev_desc(**{**good, **change})
        with pytest.raises(_lib.EngineError):
            lib.sobolev_sums(desc, *args())
        if "tabs" not in change:
            assert lib.sobolev_workspace_bytes(desc) == 0
    with pytest.raises(_lib.EngineError):
        lib.sobolev_desc(**{**good, "dims": (4, 6, 2, 2)})
    with pytest.raises(_lib.EngineError, match="workspace too small"):
        lib.sobolev_sums(lib.sobolev_desc(**good), x.data_ptr(), x.data_ptr(), ws.data_ptr(), 8, v.data_ptr(),
                         dv.data_ptr(), loss.data_ptr())
    with pytest.raises(_lib.EngineError):
        lib.sobolev_sums(lib.sobolev_desc(**good), 0, x.data_ptr(), ws.data_ptr(), 256, v.data_ptr(), dv.data_ptr(),
                         loss.data_ptr())
    with pytest.raises(_lib.EngineError):
        lib.lp_grad(lib.sobolev_desc(**{**good, "h1": False, "p": 0}), *[x.data_ptr()] * 5)
    with pytest.raises(_lib.EngineError):
        lib.lp_grad(lib.sobolev_desc(**good), *[x.data_ptr()] * 5)            # H1 has no pointwise gradient
    with pytest.raises(_lib.EngineError):
        lib.lp_grad(lib.sobolev_desc(**{**good, "h1": False}), x.data_ptr(), 0, x.data_ptr(), x.data_ptr(), x.data_ptr())
    assert float(loss) == 5.0                                              # no refused call launched anything
