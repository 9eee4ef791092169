"""Divergence-free (Helmholtz-Hodge) spectral projection on the engine: ``spectral_projection_divergence_free`` with the
call contract of the reference (neuralop/layers/spectral_projection.py:6-102) and the project's own
``HelmholtzProjection`` for 2-d and 3-d fields.

The reference transforms a real field with a full complex ``fftn``, crops the spectrum between an ``fftshift`` and an
``ifftshift``, applies ``u_hat - k (k . u_hat) / (|k|^2 + 1e-8)`` with dense wavenumber grids, zeroes "the zero mode",
pads back between two more shifts and keeps the real part of a complex ``ifftn``.  All of that is one per-mode 2 x 2
matrix ``G`` on the full FFT grid, and for real ``u``

    real(ifftn(G fftn(u))) = irfftn(G_eff rfftn(u)),     G_eff(k) = 1/2 (G(k) + G(-k mod N))      (G is real)

so the engine runs ONE real forward transform, ONE ``sc_helmholtz_project`` launch in place (sc_kernels_helmholtz.h) and
ONE inverse transform; where the crop keeps fewer modes than the grid has, both transforms are pruned to the block that
holds the kept frequencies and their mirrors.  ``G_eff`` is real, symmetric in the components and even in ``k``: the
operator is its own adjoint and the backward pass is the forward pass on the cotangent (differentiable any number of
times; nothing in a step waits for the device, so a step replays from a captured graph).

Per axis of size ``n`` with ``m = min(modes, n)`` kept and length ``L`` the shifts are index arithmetic: FFT index F is
kept iff ``0 <= c < m`` with ``c = (F + n//2) % n - (n - m)//2``; its index in the cropped spectrum is
``t = (c - m//2) % m``, it is ASSIGNED the wavenumber ``2 pi fftfreq(m, L/m)[t]`` and carries the flag ``t == 0``.
Reproduced as the reference has them:
  * where the parities of ``n`` and ``m`` differ the true zero frequency sits at ``t = 1``: every wavenumber is off by
    one step and the mode that is zeroed is frequency -1;
  * an even ``m < n`` keeps ``-m/2`` but not ``+m/2`` (``G_eff`` carries weight 1/2 at both);
  * with equal mode counts (``indexing='ij'``) component 0 takes its wavenumber from the ROW axis, built from the
    width's length, and component 1 from the column axis, built from the height's length; with unequal counts
    (``'xy'``) component 0 pairs with the column axis and component 1 with the row axis.
Different on purpose: a ``domain_size`` that is neither a number nor a pair raises ``ValueError`` (the reference dies
with an ``UnboundLocalError``); the wavenumbers are built in float64 and rounded once (the reference builds them in the
default dtype).  Not provided: Fourier continuation for non-periodic fields, half precision.

The engine takes fp32 device tensors (B, 2, H, W) with H, W >= 2; every other call -- CPU tensors, float64, complex
fields, an extent of 1 -- runs the same multiplier as a chain of torch calls.  ``route`` chooses between the two."""
import collections
import contextlib
import math

import numpy as np
import torch

from . import blocks, engine

ROUTES = ("auto", "engine", "torch")
_ROUTE = "auto"
# what "auto" does with an eligible call: the engine route is opt-in until it has been measured faster than the torch
# route at both shapes of scripts/spectral_projection_time.py (README, "Divergence-free projection")
AUTO_TAKES_ENGINE = False
REFERENCE_EPS = 1e-8
PROJECTION_EPS = 1e-30                          # HelmholtzProjection: only guards 0 / 0 at k = 0


@contextlib.contextmanager
def route(name):
    """Inside the block the projections take this route: "engine" (ValueError at a call that is not eligible), "torch"
    (the same multiplier as torch calls) or "auto" (the engine where the call is eligible and the engine has been
    measured faster, see ``AUTO_TAKES_ENGINE``)."""
    global _ROUTE
    if name not in ROUTES:
        raise ValueError(f"spectral_projection: route must be one of {ROUTES}, got {name!r}")
    saved, _ROUTE = _ROUTE, name
    try:
        yield
    finally:
        _ROUTE = saved


# ---------------------------------------------------------------------------------------------------------------------
# one axis of an operator: (kappa, keep, z) over the full FFT indices, float64
# ---------------------------------------------------------------------------------------------------------------------
def _reference_axis(n, m, length):
    """the reference's crop / shift / pad along one axis as index arithmetic (module docstring)"""
    k = 2.0 * math.pi * np.fft.fftfreq(m, d=length / m)
    kappa, keep, z = np.zeros(n), np.zeros(n), np.zeros(n)
    for f in range(n):
        c = (f + n // 2) % n - (n - m) // 2
        if 0 <= c < m:
            t = (c - m // 2) % m
            kappa[f], keep[f], z[f] = k[t], 1.0, float(t == 0)
    return kappa, keep, z


def _grid_axis(n, m, length):
    """the grid's own wavenumbers, a symmetric low-pass |f| <= (m - 1) // 2 and no Nyquist plane; no mode is zeroed"""
    kappa = 2.0 * math.pi * np.fft.fftfreq(n, d=length / n)
    f = np.abs(np.fft.fftfreq(n, d=1.0 / n).round().astype(np.int64))
    keep = np.ones(n)
    if n % 2 == 0:
        keep[n // 2] = 0.0
    if m is not None:
        keep[f > (min(int(m), n) - 1) // 2] = 0.0
    return kappa * keep, keep, np.zeros(n)


def _kept_extent(n, keep, last):
    """rows (columns) of a plan that holds every kept frequency of the axis and its mirror: 2 p + 1 (p + 1) with p the
    largest |f| among them, or the whole (half) axis where that saves no more than the Nyquist row (column)"""
    idx = np.nonzero(keep)[0]
    p = int(max([min(f, n - f) for f in idx], default=0))
    if last:
        return p + 1 if p + 1 < n // 2 else n // 2 + 1
    return 2 * p + 1 if 2 * p + 1 < n - 1 else n


def _plan_rows(n, kept, last):
    """FFT index of every row of a plan's block: 0 .. kept - 1 on the last axis, r - kept // 2 on the others"""
    return np.arange(kept) if last else (np.arange(kept) - kept // 2) % n


def _engine_tables(axes, spatial):
    """fp32 (kept_d, 2, 3) per axis: (kappa, keep, z) of the row and of its mirror"""
    out, nd = [], len(spatial)
    for d, (n, (kappa, keep, z)) in enumerate(zip(spatial, axes)):
        rows = _plan_rows(n, _kept_extent(n, keep, d == nd - 1), d == nd - 1)
        full = np.stack([kappa, keep, z], axis=-1)
        out.append(torch.from_numpy(np.stack([full[rows], full[(-rows) % n]], axis=1)).float().contiguous())
    return out


def _dense_multiplier(axes, sel, eps, spatial):
    """G (nc, nc, *spatial) on the full FFT grid, float64"""
    nd = len(spatial)
    shape = lambda d: [spatial[d] if i == d else 1 for i in range(nd)]
    w, zz = np.ones(spatial), np.ones(spatial)
    for d, (_, keep, z) in enumerate(axes):
        w = w * keep.reshape(shape(d))
        zz = zz * z.reshape(shape(d))
    w = w * (1.0 - zz)
    k = [np.broadcast_to(axes[s][0].reshape(shape(s)), spatial) for s in sel]
    den = sum(x * x for x in k) + eps
    g = np.empty((nd, nd, *spatial))
    for a in range(nd):
        for b in range(nd):
            g[a, b] = w * ((1.0 if a == b else 0.0) - k[a] * k[b] / den)
    return g


def _mirror(g, nd):
    """g(-k mod N) over the last nd axes"""
    dims = tuple(range(g.ndim - nd, g.ndim))
    return np.roll(np.flip(g, axis=dims), 1, axis=dims)


_DENSE = collections.OrderedDict()               # (key, device, dtype, half) -> the dense multiplier of the torch route
_MAX_DENSE = 8


def _torch_multiplier(key, build, device, dtype, half):
    full = (key, str(device), dtype, half)
    g = _DENSE.get(full)
    if g is None:
        axes, sel, eps, spatial = build()
        g = _dense_multiplier(axes, sel, eps, spatial)
        if half:
            g = 0.5 * (g + _mirror(g, len(spatial)))[..., :spatial[-1] // 2 + 1]
        g = torch.from_numpy(np.ascontiguousarray(g)).to(device=device, dtype=dtype)
        _DENSE[full] = g
        while len(_DENSE) > _MAX_DENSE:
            _DENSE.popitem(last=False)
    else:
        _DENSE.move_to_end(full)
    return g


def _apply_multiplier(g, uh, nd):
    """sum_b g[a, b] uh[..., b, *modes], laid out like uh.  Written as explicit sums: an einsum returns its result (and
    hands back its gradients) with the component axis innermost, a layout the transforms then have to untangle"""
    comp = lambda c: uh[(Ellipsis, c) + (slice(None),) * nd]
    g = g.to(uh.dtype)
    return torch.stack([sum(g[a, b] * comp(b) for b in range(nd)) for a in range(nd)], dim=-nd - 1)


def _project_torch(u, key, build, nd):
    """the multiplier as torch calls: (..., nd, *spatial) of any floating or complex dtype, on any device"""
    dims = tuple(range(-nd, 0))
    real = torch.empty((), dtype=u.dtype).real.dtype if u.is_complex() else u.dtype
    if u.is_complex():
        g = _torch_multiplier(key, build, u.device, real, False)
        uh = torch.fft.fftn(u, dim=dims)
        return torch.fft.ifftn(_apply_multiplier(g, uh, nd), dim=dims).real
    g = _torch_multiplier(key, build, u.device, real, True)
    uh = torch.fft.rfftn(u, dim=dims)
    return torch.fft.irfftn(_apply_multiplier(g, uh, nd), s=tuple(u.shape[-nd:]), dim=dims)


def _project_engine(u, key, build, nd):
    def tables():
        axes, sel, eps, spatial = build()
        return _engine_tables(axes, spatial), sel, eps
    tabs = engine.get_helmholtz_tables(u.device, key, tables)
    x = u.reshape(-1, nd, *u.shape[-nd:])
    return engine.HelmholtzProjectFn.apply(x.contiguous(), tabs).reshape(u.shape)


def _eligible(u, nd):
    return (torch.is_tensor(u) and u.dtype == torch.float32 and u.dim() >= nd + 1 and u.shape[-nd - 1] == nd
            and all(int(s) >= 2 for s in u.shape[-nd:]) and u.numel() > 0 and blocks._on_engine(u))


def _takes_engine(what, u, nd):
    if _ROUTE == "torch":
        return False
    if _eligible(u, nd):
        return _ROUTE == "engine" or AUTO_TAKES_ENGINE
    if _ROUTE == "engine":
        raise ValueError(f"{what}: route 'engine', but this call is not eligible for the engine (see on_engine)")
    return False


# ---------------------------------------------------------------------------------------------------------------------
# the reference's function
# ---------------------------------------------------------------------------------------------------------------------
def _domain(domain_size):
    if isinstance(domain_size, (int, float)) and not isinstance(domain_size, bool):
        return float(domain_size), float(domain_size)
    if isinstance(domain_size, (tuple, list)) and len(domain_size) == 2:
        return float(domain_size[0]), float(domain_size[1])
    raise ValueError("spectral_projection_divergence_free: domain_size must be a number or a (height, width) pair, got "
                     f"{domain_size!r}")


def _reference_operator(h, w, dh, dw, modes):
    mh, mw = min(int(modes[0]), h), min(int(modes[1]), w)
    if mh < 1 or mw < 1:
        raise ValueError(f"spectral_projection_divergence_free: constraint_modes must be positive, got {tuple(modes)}")
    if mh == mw:                         # 'ij': KX[i, j] = kx[i] (width's length) on the rows, KY = ky[j] on the columns
        return [_reference_axis(h, mh, dw), _reference_axis(w, mw, dh)], (0, 1), REFERENCE_EPS, (h, w)
    return [_reference_axis(h, mh, dh), _reference_axis(w, mw, dw)], (1, 0), REFERENCE_EPS, (h, w)


def on_engine(u, domain_size=1.0, constraint_modes=None):
    """True where ``spectral_projection_divergence_free`` with these arguments runs the engine's kernels under the
    current route (module docstring)."""
    if _ROUTE == "torch" or not (_ROUTE == "engine" or AUTO_TAKES_ENGINE):
        return False
    try:
        _domain(domain_size)
    except ValueError:
        return False
    return bool(torch.is_tensor(u) and u.dim() == 4 and _eligible(u, 2))


def spectral_projection_divergence_free(u, domain_size, constraint_modes):
    """Project a periodic 2-d velocity field onto its divergence-free part, as the reference's function.

    u (batch, 2, height, width); ``domain_size`` one length or (height, width); ``constraint_modes`` (height modes,
    width modes), clamped to the grid.  Returns the same shape and (real) dtype."""
    if u.dim() != 4:
        raise ValueError(f"spectral_projection_divergence_free: u must be (batch, 2, height, width), got "
                         f"{tuple(u.shape)}")
    dh, dw = _domain(domain_size)
    h, w = int(u.shape[2]), int(u.shape[3])
    modes = (int(constraint_modes[0]), int(constraint_modes[1]))
    key = ("reference", h, w, dh, dw, min(modes[0], h), min(modes[1], w))
    build = lambda: _reference_operator(h, w, dh, dw, modes)
    if u.shape[1] != 2:
        raise ValueError(f"spectral_projection_divergence_free: u must have 2 components, got {u.shape[1]}")
    if _takes_engine("spectral_projection_divergence_free", u, 2):
        return _project_engine(u, key, build, 2)
    if not (u.is_floating_point() or u.is_complex()):
        raise TypeError("spectral_projection_divergence_free: u must be a floating-point or complex tensor")
    return _project_torch(u, key, build, 2)


# ---------------------------------------------------------------------------------------------------------------------
# the project's own class
# ---------------------------------------------------------------------------------------------------------------------
class HelmholtzProjection:
    """Divergence-free part of a periodic vector field on a regular grid, with the conventions of ``FourierDiff``.

    ``dim`` 2 or 3: the field is (..., dim, *spatial) and component c pairs with spatial axis c.  ``L`` the domain
    length, one number or one per axis (default 2 pi); the wavenumbers are the grid's own, ``2 pi fftfreq(n, L/n)``.
    ``constraint_modes`` (one count or one per axis) is a symmetric low-pass: axis d keeps |f| <= (m_d - 1) // 2.  The
    Nyquist planes of even axes are removed -- ``FourierDiff`` differentiates them to zero, so they cannot be made
    divergence-free consistently -- and the mean flow (k = 0) is kept.  ``FourierDiff(dim, L).divergence(P(u))`` is
    zero to rounding, ``P(P(u)) = P(u)`` and ``<P u, v> = <u, P v>``."""

    def __init__(self, dim, L=None, constraint_modes=None):
        if dim not in (2, 3):
            raise ValueError("dim must be 2 or 3")
        self.dim = dim
        if L is None:
            L = 2 * math.pi
        if not isinstance(L, (tuple, list)):
            L = (L,) * dim
        if len(L) != dim:
            raise ValueError(f"For {dim}D, L must be a single float or tuple with {dim} elements")
        self.L = tuple(float(v) for v in L)
        if constraint_modes is not None:
            if not isinstance(constraint_modes, (tuple, list)):
                constraint_modes = (constraint_modes,) * dim
            if len(constraint_modes) != dim or any(int(m) < 1 for m in constraint_modes):
                raise ValueError(f"For {dim}D, constraint_modes must be one positive count or {dim} of them")
            constraint_modes = tuple(int(m) for m in constraint_modes)
        self.constraint_modes = constraint_modes

    def _operator(self, spatial):
        modes = self.constraint_modes or (None,) * self.dim
        axes = [_grid_axis(n, m, length) for n, m, length in zip(spatial, modes, self.L)]
        return axes, tuple(range(self.dim)), PROJECTION_EPS, tuple(spatial)

    def on_engine(self, u):
        """True where ``self(u)`` runs the engine's kernels under the current route"""
        if _ROUTE == "torch" or not (_ROUTE == "engine" or AUTO_TAKES_ENGINE):
            return False
        return bool(_eligible(u, self.dim))

    def __call__(self, u):
        if u.dim() < self.dim + 1 or u.shape[-self.dim - 1] != self.dim:
            raise ValueError(f"For {self.dim}D, input must be (..., {self.dim}, *spatial), got {tuple(u.shape)}")
        spatial = tuple(int(s) for s in u.shape[-self.dim:])
        key = ("grid", spatial, self.L, self.constraint_modes)
        build = lambda: self._operator(spatial)
        if _takes_engine("HelmholtzProjection", u, self.dim):
            return _project_engine(u, key, build, self.dim)
        if not (u.is_floating_point() or u.is_complex()):
            raise TypeError("HelmholtzProjection: u must be a floating-point or complex tensor")
        return _project_torch(u, key, build, self.dim)
