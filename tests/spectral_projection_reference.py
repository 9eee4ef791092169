"""TEST INFRASTRUCTURE ONLY: float64 restatements of the divergence-free spectral projection behind
``neuraloperator_amd.spectral_projection`` that do not go through the code under test.

  * ``f64_projection``: the reference function (neuralop/layers/spectral_projection.py) as ``real(ifftn(G fftn(u)))``
    with its crop / shift / pad written as index arithmetic, in torch, differentiable with autograd;
    ``f64_helmholtz``: the same for the project's own ``HelmholtzProjection``;
  * ``want_helmholtz`` / ``helmholtz_bound``: a float64 numpy evaluation of the kernel's own formula
    (sc_kernels_helmholtz.h) with arbitrary tables, and the per-element bound ``|err| <= gamma_N A``;
  * the fixture cases shared by the recorder and the tests, the kernel cases shared by the emulation and the GPU tier,
    and the runner that drives the C-ABI with free-standing descriptors between sentinel guard bands;
  * a loader for the verbatim function where it lies.  No reference source is copied here."""
import importlib.util
import math
import os

import numpy as np
import torch

from fdconv_reference import U, gamma, worst_ratio  # noqa: F401
from fourier_diff_reference import GOLDEN, crandn, default_float64  # noqa: F401
from oracle import ref_verbatim

BATCH = 2


def rel_l2(a, b):
    """|a - b| / |b| (|a| where b is zero) of real or complex tensors / arrays, in float64"""
    wide = lambda t: (t.detach().cpu().resolve_conj().numpy() if torch.is_tensor(t) else np.asarray(t))
    a, b = wide(a), wide(b)
    kind = np.complex128 if np.iscomplexobj(a) or np.iscomplexobj(b) else np.float64
    a, b = a.astype(kind), b.astype(kind)
    den = float(np.linalg.norm(b.ravel()))
    return float(np.linalg.norm((a - b).ravel())) / den if den > 0 else float(np.linalg.norm(a.ravel()))


# name -> (grid, domain_size, constraint_modes)
CASES = {
    "sproj_8x8_full": ((8, 8), 1.0, (8, 8)),
    "sproj_7x7_full_lengths": ((7, 7), (1.3, 2.9), (7, 7)),     # square modes, unequal lengths: width's k on the rows
    "sproj_8x6_full_xy": ((8, 6), (1.3, 2.9), (8, 6)),          # the 'xy' pairing
    "sproj_7x9_clamped": ((7, 9), (1.3, 2.9), (10, 12)),
    "sproj_8x8_m4x4": ((8, 8), (1.3, 2.9), (4, 4)),
    "sproj_8x8_m3x3_off_by_one": ((8, 8), (1.3, 2.9), (3, 3)),
    "sproj_7x7_m4x4": ((7, 7), (1.3, 2.9), (4, 4)),
    "sproj_9x8_m6x5": ((9, 8), (1.3, 2.9), (6, 5)),
    "sproj_8x8_m8x4_one_axis": ((8, 8), (1.3, 2.9), (8, 4)),
    "sproj_5x8_m1x1_zero": ((5, 8), (1.3, 2.9), (1, 1)),
}
EPS = 1e-8


# ---- the reference function, float64 ---------------------------------------------------------------------------------
def _axis_map(n, m, length):
    """per FFT index F of an axis: (assigned wavenumber, kept, is-the-zeroed-row), float64 tensors"""
    k = 2.0 * math.pi * torch.fft.fftfreq(m, d=length / m, dtype=torch.float64)
    kap, keep, z = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), \
        torch.zeros(n, dtype=torch.float64)
    for F in range(n):
        c = (F + n // 2) % n - (n - m) // 2
        if 0 <= c < m:
            t = (c - m // 2) % m
            kap[F], keep[F], z[F] = k[t], 1.0, 1.0 if t == 0 else 0.0
    return kap, keep, z


def f64_multiplier(h, w, domain_size, modes):
    """G (2, 2, h, w) float64 on the full FFT grid"""
    dh, dw = (float(domain_size),) * 2 if isinstance(domain_size, (int, float)) else map(float, domain_size)
    mh, mw = min(modes[0], h), min(modes[1], w)
    if mh == mw:
        k0, keep_r, z_r = _axis_map(h, mh, dw)                  # component 0: the row axis with the WIDTH's length
        k1, keep_c, z_c = _axis_map(w, mw, dh)
        K0, K1 = k0[:, None].expand(h, w), k1[None, :].expand(h, w)
    else:
        kr, keep_r, z_r = _axis_map(h, mh, dh)
        kc, keep_c, z_c = _axis_map(w, mw, dw)
        K0, K1 = kc[None, :].expand(h, w), kr[:, None].expand(h, w)
    wgt = keep_r[:, None] * keep_c[None, :] * (1.0 - z_r[:, None] * z_c[None, :])
    den = K0 * K0 + K1 * K1 + EPS
    K = (K0, K1)
    return torch.stack([torch.stack([wgt * ((1.0 if a == b else 0.0) - K[a] * K[b] / den) for b in range(2)])
                        for a in range(2)])


def apply_multiplier(g, uh):
    """sum_b g[a, b] uh[:, b] as explicit sums: an einsum returns its result, and its gradients, with the component axis
    innermost, and the FFT library of the CPU build of torch corrupts the heap on that layout at widths of 256 and up"""
    return torch.stack([sum(g[a, b] * uh[:, b] for b in range(g.shape[1])) for a in range(g.shape[0])], dim=1)


def f64_projection(u, domain_size, modes):
    """u (B, 2, h, w) real -> float64 (B, 2, h, w)"""
    u = u.double()
    g = f64_multiplier(int(u.shape[2]), int(u.shape[3]), domain_size, modes).to(torch.complex128)
    uh = torch.fft.fftn(u, dim=(2, 3))
    return torch.fft.ifftn(apply_multiplier(g, uh), dim=(2, 3)).real


def f64_helmholtz(u, dim, L=None, modes=None):
    """the project's HelmholtzProjection in float64: the grid's own wavenumbers, |f| <= (m - 1) // 2 per axis, no
    Nyquist planes, the mean kept; u (..., dim, *spatial)"""
    u = u.double()
    spatial = [int(s) for s in u.shape[-dim:]]
    L = (2 * math.pi,) * dim if L is None else ((L,) * dim if not isinstance(L, (tuple, list)) else tuple(L))
    modes = (None,) * dim if modes is None else ((modes,) * dim if not isinstance(modes, (tuple, list)) else modes)
    dims = tuple(range(-dim, 0))
    uh = torch.fft.fftn(u, dim=dims)
    ks, keep = [], torch.ones(spatial, dtype=torch.float64)
    for d, n in enumerate(spatial):
        f = torch.fft.fftfreq(n, d=1.0 / n, dtype=torch.float64)
        ok = torch.ones(n, dtype=torch.float64)
        if n % 2 == 0:
            ok[n // 2] = 0
        if modes[d] is not None:
            ok[f.abs() > (min(modes[d], n) - 1) // 2] = 0
        shape = [n if i == d else 1 for i in range(dim)]
        ks.append((2 * math.pi / L[d] * f).reshape(shape))
        keep = keep * ok.reshape(shape)
    k2 = sum(k * k for k in ks)
    comp = lambda t, c: t[(Ellipsis, c) + (slice(None),) * dim]
    kdotu = sum(ks[c] * comp(uh, c) for c in range(dim))
    safe = torch.where(k2 > 0, k2, torch.ones_like(k2))
    out = torch.stack([keep * (comp(uh, c) - ks[c] * kdotu / safe) for c in range(dim)], dim=-dim - 1)
    return torch.fft.ifftn(out.contiguous(), dim=dims).real


# ---- the verbatim function, where it exists --------------------------------------------------------------------------
def _reference_file():
    return os.path.join(ref_verbatim.REFERENCE_ROOT, "neuralop", "layers", "spectral_projection.py")


def reference_available():
    return os.path.isfile(_reference_file())


def load_reference_projection():
    """the verbatim ``spectral_projection_divergence_free``, loaded from where it lies (it imports torch and numpy only)"""
    if not reference_available():
        raise RuntimeError(f"reference not present under {ref_verbatim.REFERENCE_ROOT}")
    spec = importlib.util.spec_from_file_location("_verbatim_spectral_projection", _reference_file())
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.spectral_projection_divergence_free


def load_fixture(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def cotangent(shape, gseed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(int(gseed)), dtype=torch.float64)


def run_case(fn, u, domain_size, modes, gseed):
    """output and u.grad for the fixed random cotangent of a fixture; u a requires_grad leaf"""
    out = fn(u, domain_size, modes)
    cot = cotangent(out.shape, gseed).to(device=out.device, dtype=out.dtype)
    grad, = torch.autograd.grad((out * cot).sum(), u)
    return {"out": out.detach(), "grad": grad}


def properties(P, fd, u, v, sync=lambda: None):
    """idempotence, self-adjointness and the divergence of P(u), each as a fraction of |u|"""
    pu, pv = P(u), P(v)
    ppu = P(pu)
    div = fd.divergence(pu)
    sync()
    nu, nv = float(u.double().norm()), float(v.double().norm())
    idem = float((ppu.double() - pu.double()).norm()) / nu
    adj = abs(float((pu.double() * v.double()).sum()) - float((u.double() * pv.double()).sum())) / (nu * nv)
    return idem, adj, float(div.double().norm()) / nu


PROPERTY_GRIDS = [(7, 9), (8, 10), (8, 9), (5, 7, 9), (6, 8, 4)]


# ---- free-standing descriptors of sc_kernels_helmholtz.h through the C-ABI ---------------------------------------------
# The emulation tier (tests/test_emu_helmholtz.py) and the GPU tier (tests/test_gpu_helmholtz_kernels.py,
# device="cuda:0") run the same runner against the same float64 numpy evaluation of the kernel's own formula.
HELM_PAD_GROUPS = 16                                    # groups of guard behind the operands: the largest gpw here
SENTINEL = 7.0


def helm_tables(g, kept):
    """random host tables fp32 (kept_d, 2, 3): kappa of both signs, keep and z random 0 / 1; row 0 of every axis has
    kappa = 0, keep = 1 and z = 0 for both signs, so mode (0, .., 0) has all K = 0 and w = 1: eps alone stands in its
    denominator"""
    tabs = []
    for k in kept:
        t = torch.empty(k, 2, 3)
        t[..., 0] = 3.0 * torch.randn(k, 2, generator=g)
        t[..., 1] = (torch.rand(k, 2, generator=g) < 0.8).float()
        t[..., 2] = (torch.rand(k, 2, generator=g) < 0.3).float()
        t[0, :, 0], t[0, :, 1], t[0, :, 2] = 0.0, 1.0, 0.0
        tabs.append(t.contiguous())
    return tabs


def _mode_factors(tabs, sel, s):
    """K_c (list over components) and w over the mode grid for sign s, float64"""
    kept = tuple(int(t.shape[0]) for t in tabs)
    nd = len(kept)
    shape = lambda d: [kept[d] if i == d else 1 for i in range(nd)]
    col = lambda d, j: tabs[d][:, s, j].numpy().astype(np.float64).reshape(shape(d))
    keep, z = np.ones(kept), np.ones(kept)
    for d in range(nd):
        keep, z = keep * col(d, 1), z * col(d, 2)
    return [np.broadcast_to(col(a, 0), kept) for a in sel], keep * (1.0 - z)


def helm_multiplier(tabs, sel, eps, absolute=False):
    """1/2 (G+ + G-) (nc, nc, *kept) float64 from the fp32 table values; ``absolute``: 1/2 (|G+| + |G-|)"""
    nd = len(tabs)
    eps = float(np.float32(eps))
    total = 0.0
    for s in range(2):
        K, w = _mode_factors(tabs, sel, s)
        den = sum(k * k for k in K) + eps
        # the diagonal as (den - K_a^2) / den summed from its positive terms: 1 - K_a^2 / den cancels in float64 as well
        # (eps / den ~ 1e-10 keeps 6 digits of a difference of two numbers near 1)
        rest = lambda a: sum(K[c] * K[c] for c in range(nd) if c != a) + eps
        g = np.stack([np.stack([w * (rest(a) if a == b else -K[a] * K[b]) / den for b in range(nd)])
                      for a in range(nd)])
        total = total + 0.5 * (np.abs(g) if absolute else g)
    return total


def want_helmholtz(x, tabs, sel, eps):
    """float64: y[g, a] = sum_b 1/2 (G+_ab + G-_ab) x[g, b]"""
    return np.einsum("ab...,gb...->ga...", helm_multiplier(tabs, sel, eps), x.numpy().astype(np.complex128))


def helmholtz_bound(x, tabs, sel, eps):
    """(A, N) of one real component of one output element.  A: sum_b 1/2 (|G+_ab| + |G-_ab|) |x_b|, |x_b| the absolute
    value of that component of the source (a real multiplier never mixes real and imaginary parts).  N counted in
    sc_kernels_helmholtz.h with n = n_comp: keep / z products and w are exact (0 / 1 flags); n_a = eps + the other
    K_c^2 by fmaf, n - 1 roundings; den = fmaf(K_a, K_a, n_a), n; q = w / den, n + 1; the diagonal n_a q, 2 n + 1, is the
    longest (an off-diagonal -(K_a K_b) q has n + 3); all terms of n_a and den are positive, so none cancels.  The half
    sum of the two signs: 1.  Then one product and n - 1 fmaf per component: n.  N = 3 n + 2."""
    g = helm_multiplier(tabs, sel, eps, absolute=True)
    xn = x.numpy().astype(np.complex128)
    A = lambda part: np.einsum("ab...,gb...->ga...", g, np.abs(part))
    return A(xn.real), A(xn.imag), 3 * len(tabs) + 2


def helmholtz_plan(kept, groups):
    """(col_waves_log2, column tiles, gpw, workgroups along the groups) as sc_helmholtz_project (sc_engine.cpp) chooses"""
    kl, rows = kept[-1], int(np.prod(kept[:-1]))
    log2 = 2 if kl > 256 else 1 if kl > 128 else 0
    tiles = -(-kl // (128 << log2))
    gpw = 8
    while gpw > 1 and rows * tiles * (-(-groups // gpw)) < 2048:
        gpw >>= 1
    while -(-groups // gpw) > 65535 or rows * tiles * (-(-groups // gpw)) >= 1 << 23:
        gpw <<= 1
    return log2, tiles, gpw, -(-groups // gpw)


def check_case_plans():
    """(waves side by side as a power of two, column tiles, groups per workgroup, workgroups along the groups) of the
    cases of groups a and b: the edges they are cut for"""
    plan = {k: helmholtz_plan(c["kept"], c["groups"]) for k, c in HELMHOLTZ_KERNEL_CASES.items()}
    assert [plan[f"a_3x{kl}_g5"][:2] for kl in (1, 2, 127, 128, 129, 257, 513)] == \
        [(0, 1), (0, 1), (0, 1), (0, 1), (1, 1), (2, 1), (2, 2)]
    assert all(plan[f"b_1x5_g{g}"][2:] == (1, g) for g in (1, 2, 3, 4, 5, 8, 9, 33))
    assert plan["b_64x129_g257_two_waves_gpw8"] == (1, 1, 8, 33)           # 32 workgroups of 8 groups and one of 1


def run_helmholtz(lib, x, tabs, sel, eps=EPS, device="cpu", stream=0, inplace=False, comp_major=False, x_off=0,
                  y_off=0):
    """one sc_helmholtz_project call on tensors moved to `device`: (y (groups, nc, *kept) on the host, the guard floats
    around it).  The source is followed by HELM_PAD_GROUPS groups of zeros; the result lies in a buffer of SENTINEL
    with as many groups behind it (and, with y_off, one element in front): a group or column index past the end shows
    as a changed guard, not a fault.  ``inplace``: the result overwrites the source, whose storage is framed by
    SENTINEL on both sides.  x_off / y_off = 1 puts the operand one complex element into 16-byte aligned storage.
    ``comp_major`` lays the result out as (nc, groups, *kept)."""
    groups, nc = int(x.shape[0]), int(x.shape[1])
    kept = tuple(int(k) for k in x.shape[2:])
    modes = int(np.prod(kept))
    n = groups * nc * modes
    pad = HELM_PAD_GROUPS * nc * modes
    dev_tabs = [t.to(device) for t in tabs]
    y_gs, y_cs = (modes, groups * modes) if comp_major else (nc * modes, modes)
    call = lambda xp, yp: lib.helmholtz_project(xp, yp, kept=kept, groups=groups, sel=sel, eps=eps,
                                                tabs=[t.data_ptr() for t in dev_tabs], y_group_stride=y_gs,
                                                y_comp_stride=y_cs, stream=stream)
    if inplace:
        assert not comp_major and y_off == x_off
        buf = torch.full((2 * (2 + x_off + n + pad),), SENTINEL, dtype=torch.float32, device=device)
        assert buf.data_ptr() % 16 == 0
        lo = 2 * (2 + x_off)
        buf[lo:lo + 2 * n] = torch.view_as_real(x.reshape(-1)).reshape(-1).to(device)
        call(buf.data_ptr() + 4 * lo, buf.data_ptr() + 4 * lo)
        ys = buf.cpu()
    else:
        xs = torch.zeros(x_off + n + pad + 2, dtype=torch.complex64, device=device)
        assert xs.data_ptr() % 16 == 0
        xs[x_off:x_off + n] = x.reshape(-1).to(device)
        ys = torch.full((2 * (y_off + n + pad),), SENTINEL, dtype=torch.float32, device=device)
        assert ys.data_ptr() % 16 == 0
        lo = 2 * y_off
        call(xs.data_ptr() + 8 * x_off, ys.data_ptr() + 8 * y_off)
        ys = ys.cpu()
    y = torch.view_as_complex(ys[lo:lo + 2 * n].reshape(-1, 2).contiguous())
    y = y.view(nc, groups, *kept).transpose(0, 1) if comp_major else y.view(groups, nc, *kept)
    return y, torch.cat([ys[:lo], ys[lo + 2 * n:]])


def _helm(kept, groups, sel=None, inplace=False, comp_major=False, x_off=0, y_off=0, keep_none=False):
    return dict(kept=tuple(kept), groups=groups, sel=tuple(sel) if sel else tuple(range(len(kept))), inplace=inplace,
                comp_major=comp_major, x_off=x_off, y_off=y_off, keep_none=keep_none)


def _helm_cases():
    c = {}
    for kl in (1, 2, 127, 128, 129, 257, 513):                  # a: wave layouts, second column tile at 513
        c[f"a_3x{kl}_g5"] = _helm((3, kl), 5)
    for g in (1, 2, 3, 4, 5, 8, 9, 33):                         # b: groups per workgroup
        c[f"b_1x5_g{g}"] = _helm((1, 5), g)
    c["b_64x129_g257_two_waves_gpw8"] = _helm((64, 129), 257)
    c["c_5x6x7_three_components"] = _helm((5, 6, 7), 3, sel=(2, 0, 1))
    c["c_4x33_sel_swapped"] = _helm((4, 33), 5, sel=(1, 0))
    c["c_4x33_sel_same_axis"] = _helm((4, 33), 5, sel=(0, 0))
    c["d_3x129_in_place"] = _helm((3, 129), 5, inplace=True)
    c["d_5x6x7_in_place"] = _helm((5, 6, 7), 3, sel=(1, 2, 0), inplace=True)
    c["d_4x33_group_major"] = _helm((4, 33), 5)
    c["d_4x33_component_major"] = _helm((4, 33), 5, comp_major=True)
    for kept in ((3, 129), (7, 33), (3, 300)):                  # 8-byte aligned operands
        name = "x".join(map(str, kept))
        c[f"d_{name}_xhat_off_by_one"] = _helm(kept, 5, x_off=1)
        c[f"d_{name}_yhat_off_by_one"] = _helm(kept, 5, y_off=1)
    c["d_3x129_in_place_off_by_one"] = _helm((3, 129), 5, inplace=True, x_off=1, y_off=1)
    c["e_4x33_keep_all_zero"] = _helm((4, 33), 5, keep_none=True)
    c["e_5x6x7_keep_all_zero_in_place"] = _helm((5, 6, 7), 3, inplace=True, keep_none=True)
    return c


HELMHOLTZ_KERNEL_CASES = _helm_cases()
REPEAT_CASES = ("a_3x129_g5", "a_3x257_g5", "a_3x513_g5", "b_1x5_g9", "b_64x129_g257_two_waves_gpw8",
                "c_5x6x7_three_components", "d_3x129_in_place", "d_3x129_yhat_off_by_one")


def helm_case_inputs(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    tabs = helm_tables(g, cfg["kept"])
    if cfg["keep_none"]:
        tabs[-1][..., 1] = 0.0
    return crandn(g, cfg["groups"], len(cfg["kept"]), *cfg["kept"]), tabs


def run_helm_case(lib, cfg, inputs, device="cpu", stream=0):
    x, tabs = inputs
    return run_helmholtz(lib, x, tabs, cfg["sel"], EPS, device, stream, cfg["inplace"], cfg["comp_major"], cfg["x_off"],
                         cfg["y_off"])


def check_helm_case(name, cfg, inputs, got):
    """the two bars of a case, its exact zeros and the untouched guards; prints and returns (rel-L2, worst ratio)"""
    x, tabs = inputs
    y, around = got
    want = want_helmholtz(x, tabs, cfg["sel"], EPS)
    a_re, a_im, n = helmholtz_bound(x, tabs, cfg["sel"], EPS)
    yn = y.numpy()
    den = np.linalg.norm(want.ravel())
    rel = float(np.linalg.norm((yn - want).ravel()) / den) if den > 0 else float(np.linalg.norm(yn.ravel()))
    ratio = max(worst_ratio(yn.real, want.real, a_re, n), worst_ratio(yn.imag, want.imag, a_im, n))
    print(f"{name} plan {helmholtz_plan(cfg['kept'], cfg['groups'])} rel_l2 {rel:.1e} worst |err| / (gamma_N A) "
          f"{ratio:.3f} (N={n})")
    assert rel <= 1e-5 and ratio <= 1.0, (name, rel, ratio)
    assert torch.all(around == SENTINEL), "a value outside the result was written"
    if cfg["keep_none"]:
        assert torch.all(torch.view_as_real(y.contiguous()) == 0)
    else:
        eps_mode = (slice(None), slice(None)) + (0,) * len(cfg["kept"])     # all K = 0, w = 1: G = eps / eps
        assert rel_l2(y[eps_mode], x[eps_mode]) <= 1e-6
    return rel, ratio


def refused_helmholtz_arguments(lib, device="cpu"):
    """every refused sc_helmholtz_project argument returns its error before any launch"""
    import pytest
    from neuraloperator_amd import _lib
    g = torch.Generator().manual_seed(1)
    kept = (4, 3)
    tabs = [t.to(device) for t in helm_tables(g, kept)]
    x = crandn(g, 2, 2, *kept).to(device)
    y = torch.zeros(2, 2, *kept, dtype=torch.complex64, device=device)
    ok = dict(kept=kept, groups=2, sel=(0, 1), eps=EPS, tabs=[t.data_ptr() for t in tabs], y_group_stride=24,
              y_comp_stride=12)
    xp, yp = torch.view_as_real(x).data_ptr(), torch.view_as_real(y).data_ptr()
    lib.helmholtz_project(xp, yp, **ok)
    first = y.cpu().clone()
    bad = [dict(kept=(4, 0)), dict(kept=(4, -1)), dict(sel=(0, 2)), dict(sel=(-1, 1)), dict(eps=0.0), dict(eps=-1e-8),
           dict(eps=float("nan")), dict(groups=-1), dict(y_comp_stride=-1), dict(y_group_stride=-1),
           dict(tabs=[tabs[0].data_ptr(), 0])]
    for change in bad:
        with pytest.raises(_lib.EngineError):
            lib.helmholtz_project(xp, yp, **{**ok, **change})
    for ptrs in ((0, yp), (xp, 0)):
        with pytest.raises(_lib.EngineError):
            lib.helmholtz_project(*ptrs, **ok)
    with pytest.raises(_lib.EngineError):                                 # in place with another layout
        lib.helmholtz_project(xp, xp, **{**ok, "y_group_stride": 12, "y_comp_stride": 24})
    for nd_kept, nd_sel in (((4,), (0,)), ((2, 2, 2, 3), (0, 1, 2, 3))):  # ndim 1 and 4: the descriptor cannot hold them
        with pytest.raises(_lib.EngineError):
            lib.helmholtz_project(xp, yp, **{**ok, "kept": nd_kept, "sel": nd_sel, "tabs": [tabs[0].data_ptr()] * len(nd_kept)})
    d = _lib.HelmholtzDesc()                                              # ... and the C side refuses a raw ndim = 1
    d.ndim, d.eps, d.groups, d.kept[0], d.T[0] = 1, EPS, 2, 4, tabs[0].data_ptr()
    assert lib.lib.sc_helmholtz_project(_lib.byref(d), xp, yp, 0) != 0
    d.ndim = 4
    assert lib.lib.sc_helmholtz_project(_lib.byref(d), xp, yp, 0) != 0
    assert torch.equal(torch.view_as_real(y.cpu()), torch.view_as_real(first))   # no refused call launched anything
