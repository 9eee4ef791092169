"""Spectral derivatives on the engine: ``FourierDiff`` with the call contract of the reference
(neuralop/losses/differentiation.py:858-1360).

The reference transforms a real field with a full complex ``fftn``, multiplies by one dense ``(1j K)**order`` tensor per
requested derivative, and keeps the real part of a complex ``ifftn``; ``laplacian`` / ``gradient`` / ``divergence`` /
``curl`` repeat that per term.  For real ``u`` and any per-mode multiplier ``G`` on the full FFT grid

    real(ifftn(G fftn(u))) = irfftn(G_eff rfftn(u)),     G_eff(k) = 1/2 (G(k) + conj(G(-k mod N)))

and the reference's ``G`` is separable, ``G = prod_d F_d(i_d) (1j k_d(i_d))**o_d`` with ``F_d`` its low-pass mask along
axis d, so

    G_eff = 1/2 (prod_d a_d[i_d] + prod_d b_d[i_d]),   a_d[i] = F_d(i) m_d(i),   b_d[i] = F_d(-i mod N) conj(m_d(-i mod N)),
    m_d(i) = (1j 2 pi fftfreq(N_d, L_d / N_d)[i])**o_d

Every method here is therefore ONE real forward transform (full-spectrum plan), ONE ``sc_spectral_op`` launch that
reads each source spectrum once and writes every output spectrum from per-axis tables, and ONE inverse transform.
``G_eff`` is Hermitian, so the operator's adjoint is the same operator with ``conj(G_eff)`` and the term list
transposed: the backward pass is the forward pass again (differentiable any number of times).

Reproduced as the reference has them:
  * Nyquist planes survive only where the orders over the axes sitting at Nyquist sum to an even number;
  * the 2-d / 3-d low-pass mask ``u_h[..., cutoff:, ...] = 0`` is applied in FFT order, so it removes every negative
    frequency of that axis as well;
  * the cut-offs of axis -2 (2-d) and axis -3 (3-d) are computed from the size of the NEXT axis and vice versa
    (:1248-1253, :1317-1324);
  * 1-d runs on ``rfft`` / ``irfft`` with the mask on the half spectrum (:1186-1204).

Non-fp32 real input is computed in fp32 and returned as fp32 (as ``RealSHT`` does).  Fourier continuation
(``use_fc``) is not provided.

``FiniteDiff`` (the reference's :11-660) is the other half of the file: along one axis every one of its operators is an
N x N matrix with three interior bands and, on a non-periodic axis, two one-sided boundary rows of four entries.  The
engine holds D, D^T (orders 1 and 2) of every axis as 7-band tables built in float64 (engine.finite_diff_tables) and
every method is ONE ``sc_band_apply`` launch; ``laplacian`` / ``divergence`` / ``curl`` sum inside the kernel.  The
backward pass is the same launch with the transposed tables and the term list transposed, so it differentiates any
number of times.  One difference: a non-periodic axis shorter than 4 points raises ``ValueError`` (the reference's
boundary stencils die there with an ``IndexError``).  ``central_diff_*`` are not provided.

``get_non_uniform_fd_weights`` / ``non_uniform_fd`` (the reference's :728-855) and the class ``NonUniformFD`` are
first derivatives on a point cloud.  The reference forms ``cdist(points, points)`` (N x N), takes ``topk`` and calls
``lstsq`` on every point's (d + 1) x k system ``A w = e``; what ``lstsq`` returns there is the minimum-norm solution
``w = A^T (A A^T)^-1 e``, and its regularised form ``(A^T A + 1e-6 I) w = A^T e`` is ``A^T (A A^T + 1e-6 I)^-1 e``.  On
the engine (sc_kernels_nufd.h) that is a brute-force k-nearest-neighbour search over LDS tiles, one (d + 1) x (d + 1)
Cholesky solve per point in float64, and a gather-dot whose adjoint gathers over the transposed stencil: O(N k) memory,
the stencil built once per point set by ``NonUniformFD``.  Differences to the reference: neighbours at exactly equal
distance come in ascending index (``topk`` leaves their order open); a point whose system is singular -- collinear or
coincident neighbours -- gets all-zero weights and is listed by ``NonUniformFD.ill_posed()`` (``lstsq`` returns an
rcond-dependent truncated solution there); the solve runs in float64 whatever ``lstsq`` does in fp32.  The engine takes
fp32 device tensors, points (N, d) with d = 1..3 that need no gradient, d + 1 <= k <= 32 after the clamp, at most 8
derivative indices in [0, d), and a radius only with d <= 2; every other call -- CPU tensors, float64, d > 3, k > 32,
gradients with respect to the points -- runs the reference's formula in torch."""
import contextlib
import math

import numpy as np
import torch

from . import blocks, engine

_AXES = "xyz"


def _cutoffs(spatial, ratio):
    """FFT indices each axis' low-pass mask zeroes, restating the reference's slices literally"""
    nd = len(spatial)
    if ratio is None:
        return [set() for _ in spatial]
    if nd == 1:
        nh = spatial[0] // 2 + 1
        return [set(range(nh)[int(nh * ratio):])]                                     # :1193-1195, half spectrum
    if nd == 2:
        nx, ny = spatial
        cx, cy = int(nx * ratio), int(ny * ratio)
        return [set(range(nx)[cy:]), set(range(ny)[cx:])]                              # :1249-1253
    nx, ny, nz = spatial
    cx, cy, cz = int(nx * ratio), int(ny * ratio), int(nz * ratio)
    return [set(range(nx)[cy:]), set(range(ny)[cx:]), set(range(nz)[cz:])]             # :1318-1324


def _axis_tables(n, length, order, zeroed, last, one_d):
    """a, b of one axis and order over the plan's rows: complex128 (kept,)"""
    k = 2.0 * math.pi * np.fft.fftfreq(n, d=length / n)
    m = np.ones(n, dtype=np.complex128) if order == 0 else (1j * k) ** order
    f = np.array([0.0 if i in zeroed else 1.0 for i in range(n)])
    rows = np.arange(n // 2 + 1) if last else (np.arange(n) - n // 2) % n
    if one_d:
        # rfft / irfft: the multiplier acts on the half spectrum as it is; irfft ignores the imaginary part of the DC
        # and Nyquist coefficients, which is written into the table (a = b: G_eff = a, Hermitian)
        g = (f * m)[rows]
        g[0] = g[0].real
        if n % 2 == 0:
            g[-1] = g[-1].real
        return g, g.copy()
    neg = (-rows) % n
    return (f * m)[rows], (f * np.conj(m))[neg]


def _build_tables(spatial, lengths, ratio, orders):
    zeroed = _cutoffs(spatial, ratio)
    nd = len(spatial)
    a, b = [], []
    for d in range(nd):
        rows = [_axis_tables(spatial[d], lengths[d], o, zeroed[d], d == nd - 1, nd == 1) for o in orders[d]]
        a.append(torch.from_numpy(np.stack([r[0] for r in rows])).to(torch.complex64).contiguous())
        b.append(torch.from_numpy(np.stack([r[1] for r in rows])).to(torch.complex64).contiguous())
    return a, b


class _DiffFn(torch.autograd.Function):
    """u (groups, n_src, *spatial) fp32 -> (n_out, groups, *spatial) if out_major else (groups, n_out, *spatial):
    forward transform, multiplier pass, inverse transform.  Its adjoint is itself with the terms transposed and the
    multipliers conjugated, on the same two transforms."""

    @staticmethod
    def forward(ctx, u, tabs, terms, n_out, conj, out_major):
        ctx.tabs, ctx.terms, ctx.conj, ctx.out_major, ctx.n_src = tabs, terms, conj, out_major, int(u.shape[1])
        spatial = [int(s) for s in u.shape[2:]]
        ops = engine.EngineOps("backward")
        xh = ops.forward_transform(u, list(tabs.kept))
        yh = ops.spectral_op(xh, tabs, terms, n_out, conj, out_major)
        return ops.inverse_transform(yh, None, spatial)

    @staticmethod
    def backward(ctx, g):
        if ctx.out_major:
            g = g.transpose(0, 1)
        back = tuple((o, s, c, t) for s, o, c, t in ctx.terms)
        return _DiffFn.apply(g.contiguous(), ctx.tabs, back, ctx.n_src, not ctx.conj, False), None, None, None, None, None


class FourierDiff:
    """Fourier (spectral) derivatives of periodic fields on a regular grid: the reference's class on the engine.

    Parameters as ``neuralop.losses.differentiation.FourierDiff``: ``dim`` 1, 2 or 3 (the spatial dims are the last
    ``dim`` of the input, any leading dims); ``L`` the domain length, one number or one per axis (default 2 pi);
    ``low_pass_filter_ratio`` the reference's spectral mask.  ``use_fc`` must stay ``False``."""

    def __init__(self, dim, L=None, use_fc=False, fc_degree=4, fc_n_additional_pts=50, low_pass_filter_ratio=None):
        if dim not in [1, 2, 3]:
            raise ValueError("dim must be 1, 2, or 3")
        self.dim = dim
        if L is None:
            L = 2 * torch.pi
        if not isinstance(L, (tuple, list)):
            L = (L,) * dim
        if len(L) != dim:
            raise ValueError(f"For {dim}D, L must be a single float or tuple with {dim} elements")
        self.L = L[0] if dim == 1 else L
        self.use_fc = use_fc
        self.fc_degree = fc_degree
        self.fc_n_additional_pts = fc_n_additional_pts
        self.low_pass_filter_ratio = low_pass_filter_ratio
        self.FC = None
        if self.use_fc:
            if str(self.use_fc).lower() in ["legendre", "gram"]:
                raise NotImplementedError("Fourier continuation (use_fc='Legendre' / 'Gram') is not provided by the "
                                          "engine's FourierDiff")
            raise ValueError(f"Given FC input {self.use_fc} is not valid. Must be 'legendre' or 'gram'.")

    # ------------------------------------------------------------------------------------------ the one code path
    def _apply(self, u, n_src, terms, n_out, out_major):
        """u (..., [n_src,] *spatial); terms (src, out, coef, orders per axis) -> (n_out, groups, *spatial) if
        out_major else (groups, n_out, *spatial), and the leading shape"""
        if u is None:
            raise ValueError("Input tensor u is None")
        if u.is_complex():
            raise TypeError("FourierDiff differentiates real fields")
        spatial = tuple(int(s) for s in u.shape[-self.dim:])
        lead = tuple(u.shape[:u.dim() - self.dim - (1 if n_src else 0)])
        lengths = tuple(float(v) for v in ((self.L,) if self.dim == 1 else self.L))
        orders = tuple(tuple(sorted({int(t[3][d]) for t in terms})) for d in range(self.dim))
        if any(o < 0 for per in orders for o in per):
            raise ValueError("derivative orders must be non-negative")
        ratio = self.low_pass_filter_ratio
        key = ("fourier_diff", spatial, lengths, None if ratio is None else float(ratio), orders)
        tabs = engine.get_spectral_tables(u.device, key, lambda: _build_tables(spatial, lengths, ratio, orders))
        rows = tuple((s, o, float(c), tuple(orders[d].index(int(od[d])) for d in range(self.dim)))
                     for s, o, c, od in terms)
        x = u.float().reshape(-1, n_src or 1, *spatial)
        return _DiffFn.apply(x, tabs, rows, n_out, False, out_major), lead, spatial

    def _orders(self, derivatives):
        out = []
        for d in derivatives:
            d = (d,) if self.dim == 1 and not isinstance(d, (tuple, list)) else tuple(d)
            if len(d) != self.dim:
                raise ValueError(f"For {self.dim}D, order must be a tuple with {self.dim} elements")
            out.append(d)
        return out

    def _axis(self, axis, order):
        return tuple(order if d == axis else 0 for d in range(self.dim))

    # ------------------------------------------------------------------------------------------ public methods
    def compute_multiple_derivatives(self, u, derivatives):
        """Every derivative of the list (1-d: orders; 2-d / 3-d: one order per axis) from one transform pair; a list of
        tensors shaped like ``u``."""
        orders = self._orders(derivatives)
        if not orders:
            return []
        terms = [(0, i, 1.0, o) for i, o in enumerate(orders)]
        y, _, _ = self._apply(u, 0, terms, len(orders), True)
        return [y[i].reshape(u.shape) for i in range(len(orders))]

    def derivative(self, u, order):
        if len(order) != self.dim:
            raise ValueError(f"For {self.dim}D, order must be a tuple with {self.dim} elements")
        return self.compute_multiple_derivatives(u, [tuple(order)])[0]

    def partial(self, u, direction="x", order=1):
        if direction == "x":
            return self.dx(u, order=order)
        elif direction == "y" and self.dim >= 2:
            return self.dy(u, order=order)
        elif direction == "z" and self.dim >= 3:
            return self.dz(u, order=order)
        raise ValueError(f"Invalid direction '{direction}' for dimension {self.dim}")

    def dx(self, u, order=1):
        return self.compute_multiple_derivatives(u, [self._axis(0, order)])[0]

    def dy(self, u, order=1):
        if self.dim < 2:
            raise ValueError("dy method only available for 2D and 3D")
        return self.compute_multiple_derivatives(u, [self._axis(1, order)])[0]

    def dz(self, u, order=1):
        if self.dim < 3:
            raise ValueError("dz method only available for 3D")
        return self.compute_multiple_derivatives(u, [self._axis(2, order)])[0]

    def laplacian(self, u):
        """sum of the second derivatives, one output summed inside the multiplier pass"""
        terms = [(0, 0, 1.0, self._axis(d, 2)) for d in range(self.dim)]
        y, _, _ = self._apply(u, 0, terms, 1, True)
        return y.reshape(u.shape)

    def gradient(self, u):
        """(..., *spatial) -> (..., dim, *spatial)"""
        terms = [(0, d, 1.0, self._axis(d, 1)) for d in range(self.dim)]
        y, lead, spatial = self._apply(u, 0, terms, self.dim, False)
        return y.reshape(*lead, self.dim, *spatial)

    def divergence(self, u):
        """(..., dim, *spatial) -> (..., *spatial)"""
        if u.shape[-self.dim - 1] != self.dim:
            raise ValueError(f"For {self.dim}D, input must have {self.dim} components in the vector dimension")
        terms = [(d, 0, 1.0, self._axis(d, 1)) for d in range(self.dim)]
        y, lead, spatial = self._apply(u, self.dim, terms, 1, False)
        return y.reshape(*lead, *spatial)

    def curl(self, u):
        """2-d: (..., 2, nx, ny) -> (..., nx, ny), dv/dx - du/dy; 3-d: (..., 3, *spatial) -> the same shape"""
        if self.dim == 1:
            raise ValueError("curl not defined for 1D")
        elif self.dim == 2 and u.shape[-3] != 2:
            raise ValueError("For 2D, input must have 2 components in the vector dimension")
        elif self.dim == 3 and u.shape[-4] != 3:
            raise ValueError("For 3D, input must have 3 components in the vector dimension")
        if self.dim == 2:
            terms = [(1, 0, 1.0, (1, 0)), (0, 0, -1.0, (0, 1))]
            y, lead, spatial = self._apply(u, 2, terms, 1, False)
            return y.reshape(*lead, *spatial)
        terms = [(2, 0, 1.0, (0, 1, 0)), (1, 0, -1.0, (0, 0, 1)),        # dw/dy - dv/dz
                 (0, 1, 1.0, (0, 0, 1)), (2, 1, -1.0, (1, 0, 0)),        # du/dz - dw/dx
                 (1, 2, 1.0, (1, 0, 0)), (0, 2, -1.0, (0, 1, 0))]        # dv/dx - du/dy
        y, lead, spatial = self._apply(u, 3, terms, 3, False)
        return y.reshape(*lead, 3, *spatial)


class FiniteDiff:
    """Finite differences on a regular grid: the reference's class on the engine.

    Parameters as ``neuralop.losses.differentiation.FiniteDiff``: ``dim`` 1, 2 or 3 (the spatial dims are the last
    ``dim`` of the input, any leading dims); ``h`` the grid spacing, one number or one per axis; ``periodic_in_x/y/z``
    central differences through the wrap (True) or one-sided third-order stencils at the two ends (False)."""

    def __init__(self, dim, h=1.0, periodic_in_x=True, periodic_in_y=True, periodic_in_z=True):
        if dim not in [1, 2, 3]:
            raise ValueError("dim must be 1, 2, or 3")
        self.dim = dim
        if isinstance(h, (int, float)):
            self.h = tuple(h for _ in range(dim))
        else:
            if len(h) != dim:
                raise ValueError(f"For {dim}D, h must be a float or a tuple of length {dim}")
            self.h = tuple(h)
        self.periodic_in_x = periodic_in_x
        if dim >= 2:
            self.periodic_in_y = periodic_in_y
        if dim >= 3:
            self.periodic_in_z = periodic_in_z

    # ------------------------------------------------------------------------------------------ the one code path
    def _periodic(self):
        return tuple(bool(getattr(self, "periodic_in_" + _AXES[d])) for d in range(self.dim))

    def _apply(self, u, n_src, terms, n_out, out_major):
        """u (..., [n_src,] *spatial); terms (src, out, coef, axis, order) -> (n_out, groups, *spatial) if out_major
        else (groups, n_out, *spatial), and the leading shape"""
        if u.is_complex():
            raise TypeError("FiniteDiff differentiates real fields")
        for t in terms:
            if t[4] not in (1, 2):
                raise ValueError("Only 1st and 2nd order derivatives currently supported")
        if u.dim() < self.dim + (1 if n_src else 0):
            raise ValueError(f"FiniteDiff: a {u.dim()}-d tensor has no {self.dim} spatial dims")
        spatial = tuple(int(s) for s in u.shape[-self.dim:])
        lead = tuple(u.shape[:u.dim() - self.dim - (1 if n_src else 0)])
        periodic = self._periodic()
        for n, per in zip(spatial, periodic):
            if not per and n < 4:
                raise ValueError(f"FiniteDiff: a non-periodic axis needs at least 4 points for its one-sided boundary "
                                 f"stencils, got {n}")
        engine._require_gpu(u, "field")
        tabs = engine.finite_diff_tables(u.device, spatial, self.h, periodic)
        rows = tuple((s, o, float(c), a, od - 1) for s, o, c, a, od in terms)          # table rows: D1, D2, D1^T, D2^T
        x = u.float().reshape(-1, n_src or 1, *spatial)
        return engine.EngineOps.band_apply(x, tabs, rows, n_out, out_major), lead, spatial

    def _d(self, u, axis, order):
        y, _, _ = self._apply(u, 0, [(0, 0, 1.0, axis, order)], 1, True)
        return y.reshape(u.shape)

    # ------------------------------------------------------------------------------------------ public methods
    def dx(self, u, order=1):
        return self._d(u, 0, order)

    def dy(self, u, order=1):
        if self.dim < 2:
            raise ValueError("dy is only available for 2D and 3D")
        return self._d(u, 1, order)

    def dz(self, u, order=1):
        if self.dim < 3:
            raise ValueError("dz is only available for 3D")
        return self._d(u, 2, order)

    def laplacian(self, u):
        """sum of the second derivatives, one output summed inside the kernel"""
        y, _, _ = self._apply(u, 0, [(0, 0, 1.0, d, 2) for d in range(self.dim)], 1, True)
        return y.reshape(u.shape)

    def gradient(self, u):
        """(..., *spatial) -> (..., dim, *spatial); 1-d: du/dx shaped like u, as the reference returns it"""
        if self.dim == 1:
            return self._d(u, 0, 1)
        y, lead, spatial = self._apply(u, 0, [(0, d, 1.0, d, 1) for d in range(self.dim)], self.dim, False)
        return y.reshape(*lead, self.dim, *spatial)

    def divergence(self, u):
        """(..., dim, *spatial) -> (..., *spatial)"""
        if u.shape[-self.dim - 1] != self.dim:
            raise ValueError(f"Input must be a {self.dim}D vector field with {self.dim} components")
        y, lead, spatial = self._apply(u, self.dim, [(d, 0, 1.0, d, 1) for d in range(self.dim)], 1, False)
        return y.reshape(*lead, *spatial)

    def curl(self, u):
        """2-d: (..., 2, nx, ny) -> (..., nx, ny), dv/dx - du/dy; 3-d: (..., 3, *spatial) -> the same shape"""
        if self.dim == 1:
            raise ValueError("Curl is not defined for 1D")
        elif self.dim == 2:
            if u.shape[-3] != 2:
                raise ValueError("Input must be a 2D vector field with 2 components")
            y, lead, spatial = self._apply(u, 2, [(1, 0, 1.0, 0, 1), (0, 0, -1.0, 1, 1)], 1, False)
            return y.reshape(*lead, *spatial)
        if u.shape[-4] != 3:
            raise ValueError("Input must be a 3D vector field with 3 components")
        terms = [(2, 0, 1.0, 1, 1), (1, 0, -1.0, 2, 1),        # dw/dy - dv/dz
                 (0, 1, 1.0, 2, 1), (2, 1, -1.0, 0, 1),        # du/dz - dw/dx
                 (1, 2, 1.0, 0, 1), (0, 2, -1.0, 1, 1)]        # dv/dx - du/dy
        y, lead, spatial = self._apply(u, 3, terms, 3, False)
        return y.reshape(*lead, 3, *spatial)


# ---------------------------------------------------------------------------------------------------------------------
# finite differences on a point cloud
# ---------------------------------------------------------------------------------------------------------------------
ROUTES = ("auto", "engine", "torch")
_ROUTE = "auto"


@contextlib.contextmanager
def route(name):
    """Inside the block the point-cloud finite differences take this route: "engine" (ValueError at a call that is not
    eligible), "torch" (the reference's formula) or "auto" (the engine wherever the call is eligible)."""
    global _ROUTE
    if name not in ROUTES:
        raise ValueError(f"non_uniform_fd: route must be one of {ROUTES}, got {name!r}")
    saved, _ROUTE = _ROUTE, name
    try:
        yield
    finally:
        _ROUTE = saved


def _nufd_k(points, num_neighbors):
    return min(max(num_neighbors, 3), points.shape[0])


def on_engine(points, values=None, num_neighbors=5, derivative_indices=[0], radius=None, regularize_lstsq=False):
    """True where get_non_uniform_fd_weights / non_uniform_fd / NonUniformFD with these arguments run the engine's
    kernels (module docstring); ``values`` may be left out."""
    if _ROUTE == "torch" or not torch.is_tensor(points) or points.dim() != 2:
        return False
    tensors = [points] + ([] if values is None else [values])
    if any(t.dtype != torch.float32 for t in tensors) or not all(blocks._on_engine(t) for t in tensors):
        return False
    n, d = int(points.shape[0]), int(points.shape[1])
    if not 1 <= d <= 3 or points.requires_grad:
        return False
    if not isinstance(num_neighbors, int) or isinstance(num_neighbors, bool):
        return False
    k = _nufd_k(points, num_neighbors)
    try:
        deriv = [int(i) for i in derivative_indices]
    except (TypeError, ValueError):
        return False
    if not d + 1 <= k <= engine.NUFD_MAX_K or not 1 <= len(deriv) <= engine.NUFD_MAX_DERIV:
        return False
    if any(not 0 <= i < d for i in deriv) or (radius is not None and d > 2):
        return False
    if values is not None and (values.dim() < 1 or values.shape[-1] != n):
        return False
    return True


def _take_engine(what, *args):
    if on_engine(*args):
        return True
    if _ROUTE == "engine":
        raise ValueError(f"{what}: route 'engine', but this call is not eligible for the engine (see on_engine)")
    return False


def _weights_torch(points, num_neighbors, derivative_indices, radius, regularize_lstsq):
    """the reference's chain of torch calls (:756-812): dense distances, topk, lstsq"""
    n, d = points.shape
    k = _nufd_k(points, num_neighbors)
    nd = len(derivative_indices)
    dist, indices = torch.topk(torch.cdist(points, points, p=2), k=k, dim=1, largest=False)
    keep = torch.ones_like(dist, dtype=torch.bool)
    if radius is not None:
        keep = dist <= radius
        keep[:, :3] = True
    A = torch.ones((n, d + 1, k), dtype=points.dtype, device=points.device)
    for i in range(d):
        A[:, i + 1, :] = points[indices, i] - points[:, i].unsqueeze(1)
    A = A.unsqueeze(1).expand(-1, nd, -1, -1) * keep.unsqueeze(1).unsqueeze(2)
    b = torch.zeros((nd, d + 1, 1), dtype=points.dtype, device=points.device)
    for j, i in enumerate(derivative_indices):
        b[j, i + 1] = 1
    b = b.unsqueeze(0).expand(n, -1, -1, -1)
    if regularize_lstsq:
        At = A.transpose(-2, -1)
        gram = torch.matmul(At, A) + engine.NUFD_LAMBDA * torch.eye(k, dtype=A.dtype, device=A.device)
        w = torch.cholesky_solve(torch.matmul(At, b), torch.linalg.cholesky(gram)).squeeze(-1)
    else:
        w = torch.linalg.lstsq(A, b).solution
    return indices, w.squeeze(-1)


def get_non_uniform_fd_weights(points, num_neighbors=5, derivative_indices=[0], radius=None, regularize_lstsq=False):
    """Finite-difference weights of the first derivatives on a point cloud, as the reference's function: points (N, d),
    ``k = min(max(num_neighbors, 3), N)`` nearest neighbours per point (itself included), ``derivative_indices`` the
    coordinates to differentiate along, ``radius`` zeroes the weights of farther neighbours (the first three are always
    kept), ``regularize_lstsq`` adds 1e-6 to the normal equations.  Returns ``indices`` int64 (N, k) and ``fd_weights``
    (N, len(derivative_indices), k)."""
    if not _take_engine("get_non_uniform_fd_weights", points, None, num_neighbors, derivative_indices, radius,
                        regularize_lstsq):
        return _weights_torch(points, num_neighbors, derivative_indices, radius, regularize_lstsq)
    st = engine.NufdStencil(points, _nufd_k(points, num_neighbors), derivative_indices, radius, regularize_lstsq)
    return st.indices, st.fd_weights


def non_uniform_fd(points, values, num_neighbors=5, derivative_indices=[0], radius=None, regularize_lstsq=False):
    """First derivatives of ``values`` (N,) on the point cloud ``points`` (N, d): (len(derivative_indices), N).  Builds
    the stencil on every call, as the reference does; ``NonUniformFD`` builds it once."""
    if not _take_engine("non_uniform_fd", points, values, num_neighbors, derivative_indices, radius, regularize_lstsq):
        indices, w = _weights_torch(points, num_neighbors, derivative_indices, radius, regularize_lstsq)
        return torch.einsum("nij,nj->in", w, values[indices])
    if values.dim() != 1:
        raise ValueError(f"non_uniform_fd: values must be (N,), got {tuple(values.shape)}; NonUniformFD takes (..., N)")
    st = engine.NufdStencil(points, _nufd_k(points, num_neighbors), derivative_indices, radius, regularize_lstsq)
    return engine.NufdApplyFn.apply(values.reshape(1, -1), st)[:, 0]


class NonUniformFD:
    """First derivatives on a fixed point cloud: the stencil -- neighbour indices, weights and, on the engine, its
    transpose for the backward pass -- is built once, ``fd(values)`` applies it to ``values`` (..., N) and returns
    (n_deriv, ..., N), differentiable with respect to ``values`` through one autograd node (engine.NufdApplyFn).
    Parameters as ``get_non_uniform_fd_weights``.  Attributes: ``indices`` (N, k), ``fd_weights`` (N, n_deriv, k),
    ``k``.  On the engine neither the call nor its backward pass waits for the device, so a step replays from a captured
    graph; ``ill_posed()`` is the one call that does."""

    _MAX_BATCH = 65535

    def __init__(self, points, num_neighbors=5, derivative_indices=[0], radius=None, regularize_lstsq=False):
        self.derivative_indices = [int(i) for i in derivative_indices]
        self.k = _nufd_k(points, num_neighbors)
        self.n = int(points.shape[0])
        self._stencil = None
        if _take_engine("NonUniformFD", points, None, num_neighbors, derivative_indices, radius, regularize_lstsq):
            self._stencil = engine.NufdStencil(points, self.k, self.derivative_indices, radius, regularize_lstsq)
            self.indices, self.fd_weights = self._stencil.indices, self._stencil.fd_weights
        else:
            self.indices, self.fd_weights = _weights_torch(points, num_neighbors, self.derivative_indices, radius,
                                                           regularize_lstsq)

    def on_engine(self, values=None):
        """True where ``self(values)`` runs the engine's kernels"""
        if self._stencil is None or _ROUTE == "torch":
            return False
        return values is None or (values.dtype == torch.float32 and blocks._on_engine(values) and values.dim() >= 1
                                  and values.shape[-1] == self.n and values.device == self._stencil.device)

    def ill_posed(self):
        """indices of the points whose system was singular (all-zero weights); waits for the device.  The torch route
        flags nothing."""
        if self._stencil is None:
            return torch.empty(0, dtype=torch.int64, device=self.indices.device)
        return torch.nonzero(self._stencil.flag, as_tuple=False).reshape(-1)

    def __call__(self, values):
        if values.dim() < 1 or values.shape[-1] != self.n:
            raise ValueError(f"NonUniformFD: values must be (..., {self.n}), got {tuple(values.shape)}")
        if not self.on_engine(values):
            if _ROUTE == "engine":
                raise ValueError("NonUniformFD: route 'engine', but this call is not eligible for the engine "
                                 "(see on_engine)")
            return torch.einsum("nij,...nj->i...n", self.fd_weights.to(values.dtype), values[..., self.indices])
        lead = tuple(values.shape[:-1])
        flat = values.reshape(-1, self.n)
        parts = [engine.NufdApplyFn.apply(flat[i:i + self._MAX_BATCH], self._stencil)
                 for i in range(0, max(flat.shape[0], 1), self._MAX_BATCH)]
        out = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
        return out.reshape(len(self.derivative_indices), *lead, self.n)
