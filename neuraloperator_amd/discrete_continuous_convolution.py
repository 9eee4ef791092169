"""Equidistant discrete-continuous (DISCO) convolutions on the engine: the local integral kernel of the local neural
operator (neuralop/layers/discrete_continuous_convolution.py, EquidistantDiscreteContinuousConv2d and
EquidistantDiscreteContinuousConvTranspose2d).  Constructor arguments, defaults, assertions, errors, attributes, parameter
shapes and initial scale, the non-persistent filter buffer and the state dict are the reference's; the forward pass is
one autograd node over sc_disco_forward / sc_disco_backward (engine.DiscoConvFn) instead of an einsum that
materialises the kernel followed by conv2d / conv_transpose2d.

As in the reference the forward pass pads with zeros whatever `periodic` says (padding_mode is only an attribute), and
the filter buffer is normalised over (k0 // 2) k1 + k0 % 2 of its basis functions only.

The filter basis is torch_harmonics' where that package can be imported; otherwise it is filter_basis.py's own piecewise
linear basis, which has not been compared with torch_harmonics.  The unstructured classes (DiscreteContinuousConv2d and
its transpose, sparse Psi over point clouds) are not provided."""
import math

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, engine
from .filter_basis import basis_class


def _local_filter_matrix(kernel_shape, kernel_size, basis_type, radius_cutoff, psi_h, psi_w, q_weight, eps=1e-9):
    """(K, psi_h, psi_w) fp32: the basis functions on the grid linspace(-r, r, psi_h) x linspace(-r, r, psi_w) about the
    origin; the first (k0 // 2) k1 + k0 % 2 of them divided by their quadrature sum + eps, the others left as they are"""
    x = torch.linspace(-radius_cutoff, radius_cutoff, psi_h)
    y = torch.linspace(-radius_cutoff, radius_cutoff, psi_w)
    x, y = torch.meshgrid(x, y, indexing="ij")
    grid_in = torch.stack([x.reshape(-1), y.reshape(-1)]).reshape(2, 1, -1)
    diffs = grid_in - torch.Tensor([[0.0], [0.0]]).reshape(2, 1, 1)
    r = torch.sqrt(diffs[0] ** 2 + diffs[1] ** 2)
    phi = torch.arctan2(diffs[1], diffs[0]) + torch.pi
    idx, vals = basis_class(basis_type)(kernel_shape).compute_support_vals(r, phi, r_cutoff=radius_cutoff)
    idx = idx.permute(1, 0)
    quad = q_weight * torch.ones(psi_h * psi_w)
    q = quad[idx[2]].reshape(-1)
    for ik in range((kernel_shape[0] // 2) * kernel_shape[1] + kernel_shape[0] % 2):
        sel = torch.argwhere((idx[0] == ik) & (idx[1] == 0))
        vals[sel] = vals[sel] / (torch.sum(vals[sel] * q[sel]) + eps)
    dense = torch.zeros(kernel_size, psi_h * psi_w)
    dense[idx[0], idx[2]] = vals
    return dense.reshape(kernel_size, psi_h, psi_w)


class _EquidistantDisco(nn.Module):
    _transposed = False

    def __init__(self, in_channels, out_channels, in_shape, out_shape, kernel_shape, basis_type="piecewise_linear",
                 domain_length=None, periodic=False, groups=1, bias=True, radius_cutoff=None):
        super().__init__()
        self.kernel_shape = [kernel_shape, kernel_shape] if isinstance(kernel_shape, int) else kernel_shape
        if basis_type == "morlet":
            self.kernel_size = math.prod(self.kernel_shape)
        else:
            self.kernel_size = (self.kernel_shape[0] - 1) * self.kernel_shape[1] + 1
        self.groups = groups
        if in_channels % self.groups != 0:
            raise ValueError("Error, the number of input channels has to be an integer multiple of the group size")
        if out_channels % self.groups != 0:
            raise ValueError("Error, the number of output channels has to be an integer multiple of the group size")
        self.groupsize = in_channels // self.groups
        weight = math.sqrt(1.0 / self.groupsize) * torch.randn(out_channels, self.groupsize, self.kernel_size)
        if self._transposed:                                 # conv_transpose2d's layout: (in_channels, out_channels / groups, K)
            weight = weight.permute(1, 0, 2).reshape(self.groupsize * self.groups, -1, self.kernel_size)
        self.weight = nn.Parameter(weight)
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None

        self.padding_mode = "circular" if periodic else "zeros"
        self.domain_length = [2, 2] if domain_length is None else domain_length
        fine, coarse = (out_shape, in_shape) if self._transposed else (in_shape, out_shape)
        if radius_cutoff is None:
            radius_cutoff = max([self.domain_length[i] / float(coarse[i]) for i in (0, 1)])
        if radius_cutoff <= 0.0:
            raise ValueError("Error, radius_cutoff has to be positive.")
        # evaluated in Python floats with this expression: for some sizes the product rounds below an integer
        self.psi_local_h = math.floor(2*radius_cutoff * fine[0] / self.domain_length[0]) + 1
        self.psi_local_w = math.floor(2*radius_cutoff * fine[1] / self.domain_length[1]) + 1
        assert (fine[0] >= coarse[0]) and (fine[0] % coarse[0] == 0)
        self.scale_h = fine[0] // coarse[0]
        assert (fine[1] >= coarse[1]) and (fine[1] % coarse[1] == 0)
        self.scale_w = fine[1] // coarse[1]
        self.q_weight = self.domain_length[0] * self.domain_length[1] / fine[0] / fine[1]
        self.register_buffer("local_filter_matrix",
                             _local_filter_matrix(self.kernel_shape, self.kernel_size, basis_type, radius_cutoff,
                                                  self.psi_local_h, self.psi_local_w, self.q_weight),
                             persistent=False)

    def get_local_filter_matrix(self):
        """Psi with its two spatial axes swapped and both flipped: what the convolution kernel is formed from"""
        return self.local_filter_matrix.permute(0, 2, 1).flip(dims=(-1, -2))

    def _geometry(self):
        h_pad, w_pad = (self.psi_local_h + 1) // 2 - 1, (self.psi_local_w + 1) // 2 - 1
        if not self._transposed:
            return (h_pad, w_pad), (0, 0)
        return (h_pad, w_pad), (self.scale_h - (self.psi_local_h // 2 - h_pad) - 1,
                                self.scale_w - (self.psi_local_w // 2 - w_pad) - 1)

    def on_engine(self, x):
        """True where forward(x) is the engine's kernels: fp32 data and parameters, a support of at most 15 and a stride
        of at most 4 per axis, paddings the kernels index (sc_disco_path).  Everything else is the reference's formula
        in torch."""
        tensors = [x, self.weight, self.local_filter_matrix] + ([] if self.bias is None else [self.bias])
        if x.dim() != 4 or any(t.dtype != torch.float32 for t in tensors):
            return False
        pad, opad = self._geometry()
        d = engine.DiscoConvFn.desc(x, self.weight, self.get_local_filter_matrix(), self.groups,
                                    (self.scale_h, self.scale_w), pad, opad, self.q_weight, self._transposed)
        return _lib.get_lib().disco_path(d) != 0

    def forward(self, x):
        """x (batch, in_channels, in_shape[0], in_shape[1])"""
        pad, opad = self._geometry()
        stride = (self.scale_h, self.scale_w)
        psi = self.get_local_filter_matrix()
        if self.on_engine(x):
            return engine.DiscoConvFn.apply(x, self.weight, self.bias, psi, self.groups, stride, pad, opad,
                                            self.q_weight, self._transposed)
        kernel = torch.einsum("kxy,ogk->ogxy", psi, self.weight)
        if self._transposed:
            return F.conv_transpose2d(self.q_weight * x, kernel, self.bias, stride=stride, dilation=[1, 1],
                                      padding=pad, output_padding=opad, groups=self.groups)
        return F.conv2d(self.q_weight * x, kernel, self.bias, stride=stride, dilation=1, padding=pad,
                        groups=self.groups)


class EquidistantDiscreteContinuousConv2d(_EquidistantDisco):
    """Discrete-continuous convolution on an equidistant 2-d grid: y = conv2d(q x, sum_k Psi'[k] weight[.., k], bias)
    with stride in_shape // out_shape and zero padding (Liu-Schiaffini et al., ICML 2024; Ocampo et al., ICLR 2023).

    in_channels, out_channels : int
    in_shape, out_shape : (int, int); out_shape divides in_shape
    kernel_shape : int or [int, int]
    basis_type : 'piecewise_linear' (default), 'morlet', 'zernike' (the last two need torch_harmonics)
    domain_length : default [2, 2]
    periodic : default False (sets padding_mode only)
    groups : default 1;  bias : default True
    radius_cutoff : default max(domain_length[i] / out_shape[i])
    """
    _transposed = False


class EquidistantDiscreteContinuousConvTranspose2d(_EquidistantDisco):
    """The transposed form: y = conv_transpose2d(q x, sum_k Psi'[k] weight[.., k], bias) with stride
    out_shape // in_shape; in_shape divides out_shape; radius_cutoff defaults to max(domain_length[i] / in_shape[i]);
    the weight is stored (in_channels, out_channels / groups, K)."""
    _transposed = True
