"""Real spherical-harmonic transforms on the engine: ``RealSHT`` / ``InverseRealSHT`` with the call contract the reference
uses (neuralop/layers/spherical_convolution.py:219-281 builds them as ``RealSHT(nlat=, nlon=, lmax=, mmax=, grid=, norm=)
.to(device=...).to(dtype=...)`` and calls them on (..., nlat, nlon) resp. (..., lmax, mmax) tensors).

The reference imports them from ``torch_harmonics`` (un-vendored third party, absent here).  Their semantics are
RESTATED from the published algorithm, not pinned against the package:

  RealSHT         X[k, m] = rfft_lon(x)[k, m] / nlon                (1-d real plan, mmax <= nlon // 2 + 1 columns)
                  c[l, m] = sum_k X[k, m] 2 pi w_k Pbar_l^m(cos theta_k)
  InverseRealSHT  X[k, m] = sum_l c[l, m] Pbar_l^m(cos theta_k);  x = irfft_lon(X, n = nlon) unscaled
                  (columns past nlon // 2 + 1 are not read, as torch.fft.irfft does)

with the quadrature and normalised associated Legendre functions of spherical.py (grids "equiangular" /
"legendre-gauss", norms "ortho" / "four-pi" / "schmidt"; ``csphase=False`` drops the Condon-Shortley factor (-1)^m).
Defaults: ``lmax = nlat``, ``mmax = nlon // 2 + 1`` (the reference always passes both).  The longitude stage is the
engine's 1-d real plans, the latitude stage the Legendre kernels (sc_kernels_sht.h) against REAL fp32 tables
[l, k, m] built in float64 and kept as non-persistent buffers (module state dicts do not change).  Non-fp32 real input
is transformed in fp32 (as SpectralConv does); the coefficients are complex64 and the synthesis returns fp32.

``install_torch_harmonics()`` registers a minimal ``torch_harmonics`` module exporting these two classes, so that the
reference's ``from torch_harmonics import RealSHT, InverseRealSHT`` (and with it ``neuralop.models.SFNO``) imports.
It never shadows a real installation."""
import importlib
import math
import sys
import types

import numpy as np
import torch
from torch import nn

from . import engine
from .spherical import legendre_table, quadrature


def _table(nlat, lmax, mmax, grid, norm, csphase, analysis):
    """[l, k, m] float32: 2 pi w_k Pbar_l^m(cos theta_k) (analysis) or Pbar with the inverse normalisation"""
    theta, w = quadrature(nlat, grid)
    p = legendre_table(mmax, lmax, theta, norm, inverse=not analysis)                         # [m, l, k] float64
    if analysis:
        p = p * (2.0 * math.pi * w)[None, None, :]
    if not csphase:
        p = p * ((-1.0) ** np.arange(mmax))[:, None, None]
    return torch.from_numpy(np.ascontiguousarray(p.transpose(1, 2, 0))).to(torch.float32)


class _SHTBase(nn.Module):
    def __init__(self, nlat, nlon, lmax, mmax, grid, norm, csphase, analysis):
        super().__init__()
        self.nlat, self.nlon = int(nlat), int(nlon)
        self.lmax = int(lmax) if lmax is not None else self.nlat
        self.mmax = int(mmax) if mmax is not None else self.nlon // 2 + 1
        self.grid, self.norm, self.csphase = grid, norm, bool(csphase)
        self._engine_flags = 0            # plan flags of the longitude stage (spherical.SHT passes its layer's on)
        if min(self.nlat, self.nlon, self.lmax, self.mmax) < 1:
            raise ValueError(f"empty transform: nlat={nlat} nlon={nlon} lmax={self.lmax} mmax={self.mmax}")
        self.register_buffer("weights", _table(self.nlat, self.lmax, self.mmax, grid, norm, csphase, analysis),
                             persistent=False)

    def _apply(self, fn, *args, **kwargs):
        # .to(dtype=...) / .half() / .double() leave the table's values alone: the kernels read fp32, and a round trip
        # through 16 bits would lose precision.  A cast puts the fp32 table back on the device the move chose.
        kept = self.weights
        super()._apply(fn, *args, **kwargs)
        if self.weights.dtype != torch.float32:
            self.weights = kept.to(device=self.weights.device)
        return self

    def extra_repr(self):
        return (f"nlat={self.nlat}, nlon={self.nlon}, lmax={self.lmax}, mmax={self.mmax}, grid={self.grid!r}, "
                f"norm={self.norm!r}, csphase={self.csphase}")


class RealSHT(_SHTBase):
    """x (..., nlat, nlon) real -> c (..., lmax, mmax) complex64 (see the module docstring)."""

    def __init__(self, nlat, nlon, lmax=None, mmax=None, grid="equiangular", norm="ortho", csphase=True):
        super().__init__(nlat, nlon, lmax, mmax, grid, norm, csphase, analysis=True)
        if self.mmax > self.nlon // 2 + 1:
            raise ValueError(f"mmax = {self.mmax} exceeds the {self.nlon // 2 + 1} longitudinal modes of {self.nlon} "
                             "points")

    def forward(self, x):
        *lead, nlat, nlon = x.shape
        if (nlat, nlon) != (self.nlat, self.nlon):
            raise ValueError(f"RealSHT({self.nlat}, {self.nlon}): input grid ({nlat}, {nlon})")
        if x.is_complex():
            raise TypeError("RealSHT transforms real fields")
        lines = math.prod(int(v) for v in lead)
        ops = engine.EngineOps("forward", self._engine_flags)
        xh = ops.forward_transform(x.float().reshape(1, lines * nlat, nlon), [self.mmax])     # rfft / nlon
        c = ops.legendre_analysis(xh.reshape(lines, nlat, self.mmax), self.weights)
        return c.reshape(*lead, self.lmax, self.mmax)


class InverseRealSHT(_SHTBase):
    """c (..., lmax, mmax) complex -> x (..., nlat, nlon) float32 (see the module docstring)."""

    def __init__(self, nlat, nlon, lmax=None, mmax=None, grid="equiangular", norm="ortho", csphase=True):
        super().__init__(nlat, nlon, lmax, mmax, grid, norm, csphase, analysis=False)

    def forward(self, c):
        *lead, lmax, mmax = c.shape
        if (lmax, mmax) != (self.lmax, self.mmax):
            raise ValueError(f"InverseRealSHT(lmax={self.lmax}, mmax={self.mmax}): coefficients ({lmax}, {mmax})")
        lines = math.prod(int(v) for v in lead)
        ops = engine.EngineOps("forward", self._engine_flags)
        xh = ops.legendre_synthesis(c.reshape(lines, lmax, mmax), self.weights)               # (lines, nlat, mmax)
        keep = min(mmax, self.nlon // 2 + 1)              # irfft(n = nlon) reads the first nlon // 2 + 1 columns only
        if keep < mmax:
            xh = xh[..., :keep]
        y = ops.inverse_transform(xh.reshape(1, lines * self.nlat, keep), None, [self.nlon])
        return y.reshape(*lead, self.nlat, self.nlon)


def install_torch_harmonics():
    """Register a minimal ``torch_harmonics`` (``RealSHT`` / ``InverseRealSHT`` only) in ``sys.modules``.  Returns True
    if it did; False if ``import torch_harmonics`` already works (a real installation, or an earlier call)."""
    try:
        importlib.import_module("torch_harmonics")
        return False
    except ImportError:
        pass
    mod = types.ModuleType("torch_harmonics")
    mod.__doc__ = "neuraloperator_amd stand-in: RealSHT / InverseRealSHT on the MI355X engine (no quadrature, DISCO)"
    mod.RealSHT, mod.InverseRealSHT = RealSHT, InverseRealSHT
    mod.__all__ = ["RealSHT", "InverseRealSHT"]
    sys.modules["torch_harmonics"] = mod
    return True
