"""TEST INFRASTRUCTURE ONLY: torch stand-ins for the skip-path resample of mpu.SpatialParallelSpectralConv.

``bicubic_matrix`` is the (n_out, n_in) float64 matrix of ATen's bicubic align_corners interpolation along one dim
(fp32 index arithmetic: scale = (in - 1) / (out - 1), source index scale * dst, taps floor - 1 .. floor + 2 clamped,
cubic convolution A = -0.75); the 2-d resample is My x Mx^T.  ``PencilResampleOps`` adds the engine's
``interpolate_rows`` stage to the oracle's pencil stages.  ``spectral_resample`` restates resample.py:54-66."""
import itertools

import numpy as np
import torch

from oracle_ops import PencilOracleOps


def _cubic(t):
    a = -0.75

    def c1(x):
        return ((a + 2) * x - (a + 3)) * x * x + 1

    def c2(x):
        return ((a * x - 5 * a) * x + 8 * a) * x - 4 * a

    return [c2(t + 1), c1(t), c1(1 - t), c2(2 - t)]


def bicubic_matrix(n_in, n_out):
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    m = np.zeros((n_out, n_in))
    for d in range(n_out):
        real = np.float32(scale) * np.float32(d)
        f = int(np.floor(real))
        t = float(np.float32(real - np.float32(f)))
        for k, c in enumerate(_cubic(t)):
            m[d, min(max(f - 1 + k, 0), n_in - 1)] += c
    return torch.from_numpy(m)


def bicubic_rows(x, in_grid, out_grid, src_row0, out_row0, out_rows):
    """rows [out_row0, + out_rows) of the 2-d bicubic resample of a global grid from x = its rows [src_row0, + R)"""
    r = x.shape[2]
    my = bicubic_matrix(in_grid[0], out_grid[0])[out_row0:out_row0 + out_rows]
    outside = torch.cat([my[:, :src_row0], my[:, src_row0 + r:]], 1)
    assert float(outside.abs().sum()) == 0.0, "the rows handed to interpolate_rows miss a tap"
    my = my[:, src_row0:src_row0 + r]
    mx = bicubic_matrix(in_grid[1], out_grid[1])
    return torch.einsum("oy,bcyw,vw->bcov", my, x.double(), mx).to(x.dtype)


class PencilResampleOps(PencilOracleOps):
    """the oracle's pencil stages + interpolate_rows (float64 interpolation matrices)"""

    @staticmethod
    def interpolate_rows(x, in_grid, out_grid, src_row0, out_row0, out_rows):
        return bicubic_rows(x, in_grid, out_grid, src_row0, out_row0, out_rows)


def spectral_resample(x, out_shape):
    """resample.py:54-66: rfftn (forward norm), the corner blocks of the smaller spectrum, irfftn to the new grid"""
    nd = x.ndim - 2
    axis = list(range(2, x.ndim))
    xf = torch.fft.rfftn(x.float(), norm="forward", dim=axis)
    new = list(out_shape)
    new[-1] = new[-1] // 2 + 1
    cut = [min(i, j) for i, j in zip(new, xf.shape[-nd:])]
    out = torch.zeros([x.shape[0], x.shape[1], *new], dtype=torch.cfloat)
    idx = [((None, m // 2), (-m // 2, None)) for m in cut[:-1]] + [((None, cut[-1]),)]
    for bounds in itertools.product(*idx):
        sl = (slice(None), slice(None)) + tuple(slice(*b) for b in bounds)
        out[sl] = xf[sl]
    return torch.fft.irfftn(out, s=list(out_shape), norm="forward", dim=axis)
