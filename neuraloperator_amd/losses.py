"""Data losses on the engine: ``LpLoss`` and ``H1Loss`` with the call contract of the reference
(neuralop/losses/data_losses.py:21-491).

The reference computes a loss as a chain of torch operators: flattens, differences, powers, per-line sums, roots, a
divide and a reduction -- and for H1 one ``FiniteDiff`` call (two rolls, a subtract, a divide) per axis and operand in
front of that, then the mirror image of it all in backward.  Here a loss forward is TWO launches (``sc_sobolev_sums``:
per (line, chunk) partial sums from one read of ``y_pred`` and ``y``, then one small launch that sums the chunks in a
fixed order, forms the per-line norm, its derivative and the reduced scalar) and a loss backward ONE: H1 is quadratic,

    num_l = sum_p [e^2 + sum_j (D_j e)^2],   e = y_pred - y,        d num_l / d y_pred = 2 (I + sum_j D_j^T D_j) e

so its gradient is one ``sc_band_apply`` launch with the fused difference as its source, an identity term and one
D_j^T D_j table per axis, scaled per line by ``grad_output * d v_l / d num_l``; the Lp gradient is the pointwise
``p |e|^(p-1) sign(e)`` with the same scale.  No atomics anywhere: a step repeats bit for bit.

As in the reference: ``__call__`` is the relative loss; ``p = 1`` never takes a root; ``H1Loss.__call__`` accepts
``take_root`` and ignores it; in H1 the quadrature weights are the grid spacing handed to ``FiniteDiff``.  Differences:
the gradient goes to ``y_pred`` only (a target that requires grad raises ``NotImplementedError``), the loss node
differentiates once, ``p`` is an integer >= 1, and non-fp32 operands are computed in fp32 (the result is a 0-dim fp32
tensor).  ``HdivLoss`` and the equation losses are not provided."""
import math
import warnings

import torch
from torch.autograd.function import once_differentiable

from . import engine

_AXES = "xyz"


class _LossFn(torch.autograd.Function):
    """loss(y_pred, y): sc_sobolev_sums forward, one launch backward (sc_band_apply for H1, sc_lp_grad for Lp)"""

    @staticmethod
    def forward(ctx, x, y, d, cfg, tabs):
        ctx.in_dtype = x.dtype
        xf, yf = x.float().contiguous(), y.float().contiguous()
        sums = engine.EngineOps.sobolev_sums(xf, yf, d, tabs=tabs, **cfg)
        ctx.save_for_backward(xf, yf, sums.dv)
        ctx.d, ctx.p, ctx.tabs = d, cfg["p"], tabs
        return sums.loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, y, dv = ctx.saved_tensors
        gout = gout.float().contiguous()
        d = ctx.d
        if ctx.tabs is None:
            gx = engine.lp_grad(x, y, d, dv, gout, ctx.p)
        else:
            dims = tuple(x.shape[x.dim() - d:])
            terms = ((0, 0, 2.0, -1, 0),) + tuple((0, 0, 2.0, a, 1) for a in range(d))     # 2 (I + sum_j D_j^T D_j)
            gx = engine._band_apply(x.reshape(-1, 1, *dims), y.reshape(-1, 1, *dims), ctx.tabs, terms, 1, False,
                                    scale=dv, scale_mul=gout).reshape(x.shape)
        return (gx if ctx.in_dtype == torch.float32 else gx.to(ctx.in_dtype)), None, None, None, None


def _check_pair(x, y, d, who):
    if not (torch.is_tensor(x) and torch.is_tensor(y)):
        raise TypeError(f"{who}: tensors expected")
    if x.is_complex() or y.is_complex():
        raise TypeError(f"{who}: real fields")
    if x.shape != y.shape:
        raise ValueError(f"{who}: prediction {tuple(x.shape)} and target {tuple(y.shape)} differ in shape")
    if x.dim() < d:
        raise ValueError(f"{who}: a {x.dim()}-d tensor has no {d} spatial dims")
    if y.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError(f"{who}: the engine's loss sends its gradient to the prediction only; the target "
                                  "requires grad -- detach it")


class _DataLoss(object):
    def _setup(self, d, measure, reduction, eps):
        self.d = d
        self.eps = eps
        allowed_reductions = ["sum", "mean"]
        assert reduction in allowed_reductions, \
            f"error: expected `reduction` to be one of {allowed_reductions}, got {reduction}"
        self.reduction = reduction
        if isinstance(measure, float):
            self.measure = [measure] * self.d
        else:
            self.measure = measure

    def uniform_quadrature(self, x):
        """quadrature weights ``measure / size`` per spatial dim: the loss averages over the spatial dims"""
        quadrature = [0.0] * self.d
        for j in range(self.d, 0, -1):
            quadrature[-j] = self.measure[-j] / x.size(-j)
        return quadrature

    def reduce_all(self, x):
        return torch.sum(x) if self.reduction == "sum" else torch.mean(x)

    def _quadrature(self, x, quadrature):
        if quadrature is None:
            return self.uniform_quadrature(x)
        if isinstance(quadrature, float):
            return [quadrature] * self.d
        return quadrature


class LpLoss(_DataLoss):
    """Lp norm between two discretised d-dimensional functions (``neuralop.losses.LpLoss``): ``d`` spatial dims (the
    last ``d`` of the operands), integer order ``p``, ``measure`` of the domain (a float or one per dim), ``reduction``
    "sum" / "mean" over the leading dims, ``eps`` in the relative loss's denominator."""

    def __init__(self, d=1, p=2, measure=1.0, reduction="sum", eps=1e-8):
        super().__init__()
        if int(p) != p or p < 1:
            raise ValueError(f"LpLoss: p must be an integer >= 1 on the engine, got {p}")
        self.p = int(p)
        self._setup(d, measure, reduction, eps)

    @property
    def name(self):
        return f"L{self.p}_{self.d}Dloss"

    def _run(self, x, y, relative, take_root, konst=1.0):
        _check_pair(x, y, self.d, "LpLoss")
        cfg = dict(h1=False, p=self.p, relative=relative, take_root=bool(take_root), konst=float(konst),
                   reduce_mean=self.reduction == "mean", eps=float(self.eps))
        return _LossFn.apply(x, y, self.d, cfg, None)

    def abs(self, x, y, quadrature=None, take_root=True):
        """absolute Lp norm: (prod(quadrature) sum |x - y|^p)^(1/p) per line (no root with p = 1 or take_root=False)"""
        return self._run(x, y, False, take_root, math.prod(self._quadrature(x, quadrature)))

    def rel(self, x, y, take_root=True):
        """relative Lp norm ||x - y|| / (||y|| + eps) per line"""
        return self._run(x, y, True, take_root)

    def __call__(self, y_pred, y, **kwargs):
        if kwargs:
            warnings.warn(f"LpLoss.__call__() received unexpected keyword arguments: {list(kwargs.keys())}. "
                          "These arguments will be ignored.", UserWarning, stacklevel=2)
        return self.rel(y_pred, y)


class H1Loss(_DataLoss):
    """H1 Sobolev norm between two discretised d-dimensional functions (``neuralop.losses.H1Loss``): the L2 norm plus
    that of every first ``FiniteDiff`` derivative, periodic per axis or with one-sided boundary stencils."""

    def __init__(self, d=1, measure=1.0, reduction="sum", eps=1e-8, periodic_in_x=True, periodic_in_y=True,
                 periodic_in_z=True):
        super().__init__()
        assert d > 0 and d < 4, "Currently only implemented for 1, 2, and 3-D."
        self.periodic_in_x = periodic_in_x
        self.periodic_in_y = periodic_in_y
        self.periodic_in_z = periodic_in_z
        self._setup(d, measure, reduction, eps)

    @property
    def name(self):
        return f"H1_{self.d}DLoss"

    def _run(self, x, y, relative, take_root, quadrature):
        _check_pair(x, y, self.d, "H1Loss")
        quadrature = self._quadrature(x, quadrature)
        if len(quadrature) != self.d:
            raise ValueError(f"For {self.d}D, h must be a float or a tuple of length {self.d}")
        periodic = tuple(bool(getattr(self, "periodic_in_" + _AXES[a])) for a in range(self.d))
        dims = tuple(int(n) for n in x.shape[x.dim() - self.d:])
        for n, per in zip(dims, periodic):
            if not per and n < 4:
                raise ValueError(f"H1Loss: a non-periodic axis needs at least 4 points for its one-sided boundary "
                                 f"stencils, got {n}")
        engine._require_gpu(x, "prediction")
        tabs = engine.finite_diff_tables(x.device, dims, quadrature, periodic, kind="h1")
        cfg = dict(h1=True, p=2, relative=relative, take_root=bool(take_root), konst=float(math.prod(quadrature)),
                   reduce_mean=self.reduction == "mean", eps=float(self.eps))
        return _LossFn.apply(x, y, self.d, cfg, tabs)

    def abs(self, x, y, quadrature=None, take_root=True):
        """absolute H1 norm; ``quadrature`` (a float or one per dim) is also the grid spacing of the differences"""
        return self._run(x, y, False, take_root, quadrature)

    def rel(self, x, y, quadrature=None, take_root=True):
        """relative H1 norm ||x - y||_H1 / (||y||_H1 + eps) per line"""
        return self._run(x, y, True, take_root, quadrature)

    def __call__(self, y_pred, y, quadrature=None, take_root=True, **kwargs):
        if kwargs:
            warnings.warn(f"H1Loss.__call__() received unexpected keyword arguments: {list(kwargs.keys())}. "
                          "These arguments will be ignored.", UserWarning, stacklevel=2)
        return self.rel(y_pred, y, quadrature=quadrature)
