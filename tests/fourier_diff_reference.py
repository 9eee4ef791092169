"""TEST INFRASTRUCTURE ONLY: a float64 pure-torch restatement of the spectral-derivative operator behind
``neuraloperator_amd.FourierDiff`` that does not go through the code under test, written from the formula
``real(ifftn(G fftn(u)))`` (1-d: ``irfft(G rfft(u))``) with the reference's masks, differentiable with torch autograd;
the fixture cases shared by the recorder and the tests; and a loader for the verbatim reference class where it lies
(oracle stubs for tensorly, which ``fourier_continuation.py`` imports).  No reference source is copied here."""
import contextlib
import importlib.util
import itertools
import math
import os
import sys
import types

import torch

from oracle import ref_verbatim

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LEAD = (2, 3)
# name -> (grid, L per axis, low-pass ratio)
CASES = {
    "fourier_diff_1d_6": ((6,), (1.7,), None),
    "fourier_diff_1d_9_lp": ((9,), (2.3,), 0.6),
    "fourier_diff_2d_8x6": ((8, 6), (1.3, 2.9), None),
    "fourier_diff_2d_7x9": ((7, 9), (3.1, 0.8), None),
    "fourier_diff_2d_8x8_lp": ((8, 8), (2.0, 1.1), 0.5),
    "fourier_diff_3d_4x6x8": ((4, 6, 8), (1.5, 0.9, 2.6), None),
    "fourier_diff_3d_5x4x6_lp": ((5, 4, 6), (0.7, 2.2, 1.9), 0.75),
}


def case_orders(dim):
    """every order tuple of a fixture: 0 .. 3 per axis in 1-d and 2-d, 0 .. 2 in 3-d"""
    top = 3 if dim == 3 else 4
    return [o for o in itertools.product(range(top), repeat=dim)]


def f64_derivatives(u, dim, L, ratio, orders):
    """u (..., *spatial) real -> list of float64 tensors shaped like u, one per order tuple"""
    u = u.double()
    L = (L,) * dim if not isinstance(L, (tuple, list)) else tuple(L)
    n = [int(s) for s in u.shape[-dim:]]
    if dim == 1:
        uh = torch.fft.rfft(u, dim=-1)
        k = torch.fft.rfftfreq(n[0], d=L[0] / n[0], dtype=torch.float64) * (2 * math.pi)
        mask = torch.ones(uh.shape[-1], dtype=torch.float64)
        if ratio is not None:
            mask[int(uh.shape[-1] * ratio):] = 0
        uh = uh * mask
        return [torch.fft.irfft(((1j * k) ** o[0]) * uh, dim=-1, n=n[0]) for o in orders]
    dims = tuple(range(-dim, 0))
    uh = torch.fft.fftn(u, dim=dims)
    ks = [torch.fft.fftfreq(n[d], d=L[d] / n[d], dtype=torch.float64) * (2 * math.pi) for d in range(dim)]
    if ratio is not None:
        cut = [int(n[d] * ratio) for d in range(dim)]
        # the reference cuts the first two spatial axes at each other's cut-off; the mask is one-sided (FFT order)
        cut[0], cut[1] = cut[1], cut[0]
        for d in range(dim):
            m = torch.ones(n[d], dtype=torch.float64)
            m[cut[d]:] = 0
            uh = uh * m.reshape([-1] + [1] * (dim - 1 - d))
    out = []
    for o in orders:
        g = torch.ones((), dtype=torch.complex128)
        for d in range(dim):
            g = g * ((1j * ks[d]) ** o[d]).reshape([-1] + [1] * (dim - 1 - d))
        out.append(torch.fft.ifftn(g * uh, dim=dims).real)
    return out


def _axis(dim, d, o):
    return tuple(o if i == d else 0 for i in range(dim))


class F64FourierDiff:
    """the class's methods on f64_derivatives (float64 whatever the input dtype)"""

    def __init__(self, dim, L=None, low_pass_filter_ratio=None):
        self.dim, self.L, self.ratio = dim, (2 * math.pi if L is None else L), low_pass_filter_ratio

    def compute_multiple_derivatives(self, u, derivatives):
        orders = [(o,) if self.dim == 1 and not isinstance(o, (tuple, list)) else tuple(o) for o in derivatives]
        return f64_derivatives(u, self.dim, self.L, self.ratio, orders)

    def derivative(self, u, order):
        return self.compute_multiple_derivatives(u, [tuple(order)])[0]

    def _d(self, u, d, order):
        return self.derivative(u, _axis(self.dim, d, order))

    def dx(self, u, order=1):
        return self._d(u, 0, order)

    def dy(self, u, order=1):
        return self._d(u, 1, order)

    def dz(self, u, order=1):
        return self._d(u, 2, order)

    def partial(self, u, direction="x", order=1):
        return self._d(u, "xyz".index(direction), order)

    def laplacian(self, u):
        return sum(self._d(u, d, 2) for d in range(self.dim))

    def gradient(self, u):
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


def reference_available():
    return os.path.isfile(os.path.join(ref_verbatim.REFERENCE_ROOT, "neuralop", "losses", "differentiation.py"))


def load_reference_differentiation():
    """the verbatim ``neuralop.losses.differentiation`` module, loaded from where it lies"""
    name = "neuralop.losses.differentiation"
    if name in sys.modules:
        return sys.modules[name]
    if not reference_available():
        raise RuntimeError(f"reference not present under {ref_verbatim.REFERENCE_ROOT}")
    from oracle import tl_stub
    tl_stub.install()
    root = os.path.join(ref_verbatim.REFERENCE_ROOT, "neuralop")
    for pkg, sub in (("neuralop", ""), ("neuralop.layers", "layers"), ("neuralop.losses", "losses")):
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = [os.path.join(root, sub) if sub else root]
            sys.modules[pkg] = m
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "losses", "differentiation.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


@contextlib.contextmanager
def default_float64():
    """The reference builds its frequencies with ``torch.fft.fftfreq(n, d)`` in the DEFAULT dtype: its float64 result
    is what it computes with float64 as the default (under float32 its multipliers are rounded to fp32 whatever the
    input's dtype)."""
    saved = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(saved)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    den = float(b.norm())
    return float((a - b).norm()) / den if den > 0 else float(a.norm())


def run_all(fd, u, v, gseed, dim):
    """Every method of a FourierDiff-like object ``fd`` on u / v (requires_grad leaves), with ``u.grad`` / ``v.grad``
    for fixed random cotangents.  Returns a dict name -> tensor; used on the reference (recording), the helper-free
    engine class and the verbatim class alike."""
    orders = case_orders(dim)
    out = {}
    arg = [o[0] for o in orders] if dim == 1 else orders
    many = fd.compute_multiple_derivatives(u, arg)
    out["multi"] = torch.stack(list(many), dim=0)
    out["laplacian"] = fd.laplacian(u)
    out["gradient"] = fd.gradient(u)
    out["dx2"] = fd.dx(u, order=2)
    out["partial_last"] = fd.partial(u, direction="xyz"[dim - 1], order=1)
    out["derivative"] = fd.derivative(u, tuple(range(1, dim + 1)))
    out["divergence"] = fd.divergence(v)
    if dim > 1:
        out["curl"] = fd.curl(v)
    g = torch.Generator().manual_seed(gseed)
    cot = {k: torch.randn(t.shape, generator=g, dtype=torch.float64).to(device=t.device, dtype=t.dtype)
           for k, t in sorted(out.items())}
    scal = sum((out[k] * cot[k]).sum() for k in ("multi", "laplacian", "gradient", "dx2", "partial_last", "derivative"))
    vec = sum((out[k] * cot[k]).sum() for k in ("divergence", "curl") if k in out)
    gu, = torch.autograd.grad(scal, u)
    gv, = torch.autograd.grad(vec, v)
    res = {k: t.detach() for k, t in out.items()}
    res["grad_u"], res["grad_v"] = gu, gv
    return res


# ---- free-standing descriptors of sc_kernels_specop.h through the C-ABI ------------------------------------------------
# The emulation tier (tests/test_emu_specop.py) and the GPU tier (tests/test_gpu_specop_kernels.py, device="cuda:0") run
# the same runner against the same float64 numpy evaluation of the kernel's own formula with random complex tables.
import numpy as np  # noqa: E402

from fdconv_reference import U, gamma, worst_ratio  # noqa: E402,F401

SPECOP_PAD_GROUPS = 16                                  # groups of sentinel behind the result: the largest gpw here


def crandn(g, *shape):
    return torch.complex(torch.randn(*shape, generator=g), torch.randn(*shape, generator=g))


def spec_tables(g, kept, n_tab):
    """random host tables, engine.SpectralTables: a[d], b[d] complex64 (n_tab_d, kept_d)"""
    from neuraloperator_amd import engine
    a = [crandn(g, n, k).contiguous() for n, k in zip(n_tab, kept)]
    b = [crandn(g, n, k).contiguous() for n, k in zip(n_tab, kept)]
    return engine.SpectralTables(a, b)


def spec_terms(g, n_src, n_out, n_tab, n_terms, empty=None):
    """random terms; every output but `empty` gets at least one"""
    ri = lambda hi: int(torch.randint(0, hi, (1,), generator=g))
    outs = [o for o in range(n_out) if o != empty]
    terms = []
    for j in range(n_terms):
        out = outs[j] if j < len(outs) else outs[ri(len(outs))]
        terms.append((ri(n_src), out, float(torch.randn(1, generator=g)), tuple(ri(n) for n in n_tab)))
    return tuple(terms)


def want_spectral_op(x, tabs, terms, n_out, conj):
    """float64: y[g, t] = sum coef 1/2 (prod a + prod b) x[g, src]"""
    x = x.numpy().astype(np.complex128)
    kept = x.shape[2:]
    y = np.zeros((x.shape[0], n_out) + kept, dtype=np.complex128)
    for src, out, coef, tab in terms:
        pa = np.ones(kept, dtype=np.complex128)
        pb = np.ones(kept, dtype=np.complex128)
        for d, r in enumerate(tab):
            shp = [1] * len(kept)
            shp[d] = kept[d]
            pa = pa * tabs.a[d][r].numpy().astype(np.complex128).reshape(shp)
            pb = pb * tabs.b[d][r].numpy().astype(np.complex128).reshape(shp)
        gm = float(np.float32(coef)) * 0.5 * (pa + pb)
        y[:, out] += (np.conj(gm) if conj else gm) * x[:, src]
    return y


def spectral_op_bound(x, tabs, terms, n_out):
    """(A, N) of one component of one output element.  A: with |z|_1 = |re z| + |im z|, the sum over the terms of
    |coef| / 2 (prod_d |a_d|_1 + prod_d |b_d|_1) |x|_1 -- every real product that enters either component, in absolute
    value.  N, counted in k_spectral_op: a cf_mul is a rounded product and a rounded sum (2) and the multiplier takes
    ndim of them (coef a_row0, a_row1, a_last), the cf_mac that adds the b product 2 more; then two fmaf per term into
    either component of the accumulator: 2 ndim + 2 + 2 (terms of the longest output)."""
    one = lambda t: np.abs(t.real) + np.abs(t.imag)
    xn = one(x.numpy().astype(np.complex128))
    kept = xn.shape[2:]
    A = np.zeros((xn.shape[0], n_out) + kept)
    for src, out, coef, tab in terms:
        pa, pb = np.ones(kept), np.ones(kept)
        for d, r in enumerate(tab):
            shp = [1] * len(kept)
            shp[d] = kept[d]
            pa = pa * one(tabs.a[d][r].numpy().astype(np.complex128)).reshape(shp)
            pb = pb * one(tabs.b[d][r].numpy().astype(np.complex128)).reshape(shp)
        A[:, out] += abs(float(np.float32(coef))) * 0.5 * (pa + pb) * xn[:, src]
    longest = max([sum(1 for t in terms if t[1] == o) for o in range(n_out)] + [1])
    return A, 2 * len(kept) + 2 + 2 * longest


def specop_plan(kept, groups):
    """(col_waves_log2, column tiles, gpw, workgroups along the groups) as sc_spectral_op (sc_engine.cpp) chooses them"""
    kl, rows = kept[-1], int(np.prod(kept[:-1]))
    log2 = 2 if kl > 256 else 1 if kl > 128 else 0
    tiles = -(-kl // (128 << log2))
    gpw = 8
    while gpw > 1 and rows * tiles * (-(-groups // gpw)) < 2048:
        gpw >>= 1
    while -(-groups // gpw) > 65535 or rows * tiles * (-(-groups // gpw)) >= 1 << 23:
        gpw <<= 1
    return log2, tiles, gpw, -(-groups // gpw)


def run_spectral_op(lib, x, tabs, terms, n_out, conj=False, out_major=False, device="cpu", stream=0, x_off=0, y_off=0,
                    sentinel=7.0):
    """one sc_spectral_op call on tensors moved to `device`: (y (groups, n_out, *kept) on the host, the sentinel floats
    around it).  x_off / y_off = 1 puts the spectrum one complex element into 16-byte aligned storage.  The source is
    followed by SPECOP_PAD_GROUPS groups of zeros and the result lies in a buffer of `sentinel` with SPECOP_PAD_GROUPS
    groups behind it (and, with y_off, one element in front): a group or column index past the end shows as a changed
    sentinel, not a fault."""
    groups, n_src = int(x.shape[0]), int(x.shape[1])
    kept = tuple(int(k) for k in x.shape[2:])
    modes = int(np.prod(kept))
    pad = SPECOP_PAD_GROUPS * max(n_src, n_out) * modes
    xs = torch.zeros(x.numel() + pad + 2, dtype=torch.complex64, device=device)
    assert xs.data_ptr() % 16 == 0
    xs[x_off:x_off + x.numel()] = x.reshape(-1).to(device)
    n_y = groups * n_out * modes
    ys = torch.full((2 * (y_off + n_y + pad),), sentinel, dtype=torch.float32, device=device)
    assert ys.data_ptr() % 16 == 0
    a, b = [t.to(device) for t in tabs.a], [t.to(device) for t in tabs.b]
    y_gs, y_os = (modes, groups * modes) if out_major else (n_out * modes, modes)
    lib.spectral_op(xs.data_ptr() + 8 * x_off, ys.data_ptr() + 8 * y_off, kept=kept, groups=groups, n_src=n_src, n_out=n_out, terms=terms, tabs_a=[t.data_ptr() for t in a],
                    tabs_b=[t.data_ptr() for t in b], n_tab=tabs.n_tab, y_group_stride=y_gs, y_out_stride=y_os,
                    conj=conj, stream=stream)
    ys = ys.cpu()
    lo = 2 * y_off
    y = torch.view_as_complex(ys[lo:lo + 2 * n_y].reshape(-1, 2).contiguous())
    y = y.view(n_out, groups, *kept).transpose(0, 1) if out_major else y.view(groups, n_out, *kept)
    return y, torch.cat([ys[:lo], ys[lo + 2 * n_y:]])


def _spec(kept, groups, n_src=2, n_out=2, n_terms=3, empty=None, conj=False, out_major=False, n_tab=2, x_off=0, y_off=0):
    return dict(kept=tuple(kept), groups=groups, n_src=n_src, n_out=n_out, n_terms=n_terms, empty=empty, conj=conj,
                out_major=out_major, n_tab=n_tab, x_off=x_off, y_off=y_off)


def _spec_cases():
    c = {}
    for kl in (1, 2, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025):   # a: wave layouts, second column tile at 513
        c[f"a_3x{kl}_g5"] = _spec((3, kl), 5)
    for g in (1, 2, 3, 4, 5, 7, 8, 9, 33):                                 # b: groups per workgroup falls to 1
        c[f"b_5_g{g}"] = _spec((5,), g)
    c["b_64x129_g257_two_waves_gpw8"] = _spec((64, 129), 257, n_src=1, n_out=1, n_terms=1)
    c["b_64x257_g67_four_waves_gpw2"] = _spec((64, 257), 67, n_src=1, n_out=1, n_terms=1)
    c["c_2_g524281_gpw16"] = _spec((2,), 8 * 65535 + 1, n_src=1, n_out=1, n_terms=1)      # c: the grid limit
    c["d_twelve_slots_three_sources"] = _spec((4, 33), 5, n_src=3, n_out=3, n_terms=12, n_tab=3)
    c["d_termless_output"] = _spec((4, 33), 5, n_src=2, n_out=3, n_terms=5, empty=1)
    c["d_conj"] = _spec((4, 33), 5, n_src=2, n_out=2, n_terms=4, conj=True)
    c["d_out_major"] = _spec((4, 33), 5, n_src=2, n_out=3, n_terms=5, out_major=True)
    c["d_5x6x7_two_row_axes"] = _spec((5, 6, 7), 3, n_src=2, n_out=2, n_terms=6, n_tab=4, conj=True)
    for kept in ((5,), (3, 129), (7, 33), (3, 300)):                       # e: 8-byte aligned operands
        name = "x".join(map(str, kept))
        c[f"e_{name}_xhat_off_by_one"] = _spec(kept, 5, n_terms=4, x_off=1)
        c[f"e_{name}_yhat_off_by_one"] = _spec(kept, 5, n_terms=4, y_off=1)
    return c


SPECOP_KERNEL_CASES = _spec_cases()
EMU_SPECOP_KERNEL_CASES = ("a_3x2_g5", "a_3x127_g5", "a_3x128_g5", "a_3x129_g5", "a_3x257_g5", "a_3x513_g5", "b_5_g3",
                           "b_5_g9", "b_64x257_g67_four_waves_gpw2",
                           "d_twelve_slots_three_sources", "d_5x6x7_two_row_axes", "e_3x129_xhat_off_by_one",
                           "e_3x129_yhat_off_by_one", "e_5_yhat_off_by_one")


def specop_case_inputs(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    n_tab = (cfg["n_tab"],) * len(cfg["kept"])
    tabs = spec_tables(g, cfg["kept"], n_tab)
    terms = spec_terms(g, cfg["n_src"], cfg["n_out"], n_tab, cfg["n_terms"], cfg["empty"])
    return crandn(g, cfg["groups"], cfg["n_src"], *cfg["kept"]), tabs, terms


def run_specop_case(lib, cfg, inputs, device="cpu", stream=0):
    x, tabs, terms = inputs
    return run_spectral_op(lib, x, tabs, terms, cfg["n_out"], cfg["conj"], cfg["out_major"], device, stream,
                           cfg["x_off"], cfg["y_off"])


def check_specop_case(name, cfg, inputs, got):
    """the two bars of a case, its zero output and the untouched sentinels; prints and returns (rel-L2, worst ratio)"""
    x, tabs, terms = inputs
    y, around = got
    want = want_spectral_op(x, tabs, terms, cfg["n_out"], cfg["conj"])
    A, n = spectral_op_bound(x, tabs, terms, cfg["n_out"])
    yn = y.numpy()
    rel = float(np.linalg.norm((yn - want).ravel()) / np.linalg.norm(want.ravel()))
    ratio = max(worst_ratio(yn.real, want.real, A, n), worst_ratio(yn.imag, want.imag, A, n))
    print(f"{name} plan {specop_plan(cfg['kept'], cfg['groups'])} rel_l2 {rel:.1e} worst |err| / (gamma_N A) {ratio:.3f} "
          f"(N={n})")
    assert rel <= 1e-5 and ratio <= 1.0, (name, rel, ratio)
    assert torch.all(around == 7.0), "a value outside the result was written"
    if cfg["empty"] is not None:
        assert torch.all(torch.view_as_real(y[:, cfg["empty"]].contiguous()) == 0)
    return rel, ratio


def refused_specop_arguments(lib, device="cpu"):
    """every refused sc_spectral_op argument returns its error before any launch"""
    import pytest
    from neuraloperator_amd import _lib
    g = torch.Generator().manual_seed(1)
    kept, n_tab = (4, 3), (2, 2)
    tabs = spec_tables(g, kept, n_tab)
    a, b = [t.to(device) for t in tabs.a], [t.to(device) for t in tabs.b]
    x = crandn(g, 2, 2, *kept).to(device)
    y = torch.zeros(2, 2, *kept, dtype=torch.complex64, device=device)
    ok = dict(kept=kept, groups=2, n_src=2, n_out=2, terms=((0, 0, 1.0, (0, 0)), (1, 1, 1.0, (1, 1))),
              tabs_a=[t.data_ptr() for t in a], tabs_b=[t.data_ptr() for t in b], n_tab=n_tab,
              y_group_stride=24, y_out_stride=12)
    xp, yp = torch.view_as_real(x).data_ptr(), torch.view_as_real(y).data_ptr()
    lib.spectral_op(xp, yp, **ok)
    first = y.cpu().clone()
    bad = [dict(kept=(4, 0)), dict(kept=(4, 3, 2, 2)), dict(n_src=4), dict(n_src=0), dict(n_out=0), dict(n_out=13),
           dict(groups=-1), dict(n_tab=(2, 0)), dict(terms=((2, 0, 1.0, (0, 0)),)), dict(terms=((0, 2, 1.0, (0, 0)),)),
           dict(terms=((0, 0, 1.0, (0, 2)),)), dict(terms=((0, 0, 1.0, (0, 0)),) * 13), dict(y_out_stride=-1),
           dict(n_out=12, terms=((0, 0, 1.0, (0, 0)),) * 2),            # 2 terms + 11 term-less outputs > 12 slots
           dict(tabs_a=[0, 0])]
    for change in bad:
        with pytest.raises(_lib.EngineError):
            lib.spectral_op(xp, yp, **{**ok, **change})
    lib.spectral_op(0, 0, **{**ok, "groups": 0})                      # no groups: nothing to do, no pointer read
    assert torch.equal(torch.view_as_real(y.cpu()), torch.view_as_real(first))   # no refused call launched anything
