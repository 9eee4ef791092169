"""Filter bases of the discrete-continuous convolutions.

The reference takes PiecewiseLinearFilterBasis, MorletFilterBasis and ZernikeFilterBasis from
``torch_harmonics.filter_basis``.  Where that package can be imported the layers use its classes (basis_class); where it
cannot, this module provides a piecewise linear basis of its own, WRITTEN FROM THE DEFINITION BELOW AND NOT COMPARED
WITH torch_harmonics, and the other two names raise NotImplementedError.

PiecewiseLinearFilterBasis([nr, nphi]) has K = (nr - 1) nphi + 1 functions of the polar coordinates (r, phi) of a point
relative to the output point, with dr = r_cutoff / (nr - 1), dphi = 2 pi / nphi and hat(d, width) = max(0, 1 - |d| / width):

  basis 0        hat(r, dr)                                                      the radial hat at r = 0
  basis k >= 1   hat(r - ((k - 1) // nphi + 1) dr, dr) * hat(ang(phi - ((k - 1) % nphi) dphi), dphi)
                 with ang(.) the angular distance modulo 2 pi, in [0, pi]

An entry is kept iff its value is non-zero and r <= r_cutoff.  Host code, used at construction time only."""
import math

import torch


class PiecewiseLinearFilterBasis:
    def __init__(self, kernel_shape):
        if isinstance(kernel_shape, int):
            kernel_shape = [kernel_shape, kernel_shape]
        if len(kernel_shape) != 2 or kernel_shape[0] < 1 or kernel_shape[1] < 1:
            raise ValueError(f"kernel_shape must be [nr, nphi] with positive entries, got {kernel_shape}")
        self.kernel_shape = list(kernel_shape)

    @property
    def kernel_size(self):
        return (self.kernel_shape[0] - 1) * self.kernel_shape[1] + 1

    def compute_support_vals(self, r, phi, r_cutoff):
        """r, phi (n_out, n_in): polar coordinates of every input point about every output point.  Returns
        idx (nnz, 3) int64 rows (basis, out, in) in argwhere order and vals (nnz,)."""
        nr, nphi = self.kernel_shape
        dr = r_cutoff / (nr - 1) if nr > 1 else r_cutoff
        dphi = 2.0 * math.pi / nphi
        vals = torch.zeros((self.kernel_size, *r.shape), dtype=r.dtype)
        vals[0] = (1.0 - r / dr).clamp(min=0.0)
        for k in range(1, self.kernel_size):
            ir, iphi = (k - 1) // nphi + 1, (k - 1) % nphi
            d = torch.remainder(phi - iphi * dphi, 2.0 * math.pi)
            d = torch.minimum(d, 2.0 * math.pi - d)
            vals[k] = (1.0 - (r - ir * dr).abs() / dr).clamp(min=0.0) * (1.0 - d / dphi).clamp(min=0.0)
        keep = (vals != 0) & (r <= r_cutoff).unsqueeze(0)
        idx = torch.argwhere(keep)
        return idx, vals[keep]


_OWN = {"piecewise_linear": PiecewiseLinearFilterBasis}


def basis_class(basis_type):
    """the class behind a basis name: torch_harmonics' own where the package can be imported, else this module's"""
    names = {"piecewise_linear": "PiecewiseLinearFilterBasis", "morlet": "MorletFilterBasis",
             "zernike": "ZernikeFilterBasis"}
    assert basis_type in names, f"Error: expected one of {list(names)}, got {basis_type}"
    try:
        from torch_harmonics import filter_basis as real
        return getattr(real, names[basis_type])
    except ImportError:
        pass
    if basis_type not in _OWN:
        raise NotImplementedError(f"the {basis_type!r} filter basis needs the torch_harmonics package "
                                  "(torch_harmonics.filter_basis), which cannot be imported")
    return _OWN[basis_type]
