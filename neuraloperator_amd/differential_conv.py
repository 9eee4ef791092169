"""FiniteDifferenceConvolution on the engine (the layer of neuralop/layers/differential_conv.py): the differential
branch of the local neural operator block.  Constructor arguments, defaults, errors, attributes, parameter
initialisation and state dict are the reference's; the forward pass is one autograd node over sc_fdconv_forward /
sc_fdconv_backward -- one convolution with folded weights instead of a k^d convolution, a 1 x 1 convolution of the
summed kernel, a subtraction and a division."""
import numbers

import torch
import torch.nn.functional as F
from torch import nn

from . import engine

# the reference's `padding` argument -> (torch padding_mode it stores, the engine's name)
_MODES = {"periodic": "circular", "replicate": "replicate", "reflect": "reflect", "zeros": "zeros"}
_ENGINE_MODE = {"circular": "periodic", "replicate": "replicate", "reflect": "reflect", "zeros": "zeros"}


class FiniteDifferenceConvolution(nn.Module):
    """y = (conv(x, W) - conv_1x1(x, sum of W over its taps)) / grid_width on a regular grid of n_dim dimensions; as
    the grid is refined the stencil converges to a directional derivative (Liu-Schiaffini et al., ICML 2024).

    in_channels, out_channels, n_dim : int
    kernel_size : odd int, default 3
    groups : int, default 1
    padding : 'periodic' (default), 'replicate', 'reflect' or 'zeros'
    """

    def __init__(self, in_channels, out_channels, n_dim, kernel_size=3, groups=1, padding="periodic"):
        super().__init__()
        conv_cls = getattr(nn, f"Conv{n_dim}d")
        self.F_conv_module = self.conv_function = getattr(F, f"conv{n_dim}d")
        assert kernel_size % 2 == 1, "Kernel size should be odd"
        if padding not in _MODES:
            raise NotImplementedError("Desired padding mode is not currently supported")
        self.kernel_size, self.pad_size = kernel_size, kernel_size // 2
        self.in_channels, self.groups, self.n_dim = in_channels, groups, n_dim
        self.padding_mode = _MODES[padding]
        # torch's own module holds the parameter, so initialisation and checkpoint layout are the reference's
        self.conv = conv_cls(in_channels, out_channels, kernel_size=kernel_size, groups=groups, bias=False,
                             padding="same", padding_mode=self.padding_mode)
        # one Parameter under two names: state_dict() lists conv.weight and weight, named_parameters() only weight
        self.weight = self.conv.weight

    def on_engine(self, x, grid_width):
        """True where forward(x, grid_width) is the engine's kernels: fp32 data, a plain number as grid_width, at most
        three dimensions, a stencil of 3, 5 or 7 points.  Everything else is the reference's formula in torch, a grid_width
        of 0 included (its division gives inf / nan there, as in the reference)."""
        return (x.dtype == torch.float32 and self.weight.dtype == torch.float32 and x.dim() == self.n_dim + 2
                and isinstance(grid_width, numbers.Real) and not isinstance(grid_width, bool) and grid_width != 0
                and self.n_dim <= 3 and 3 <= self.kernel_size <= 7)

    def forward(self, x, grid_width):
        """x (batch, in_channels, d_1, ..., d_n); grid_width: the spacing of the input grid"""
        if self.on_engine(x, grid_width):
            return engine.FdConvFn.apply(x, self.weight, self.groups, _ENGINE_MODE[self.padding_mode], grid_width)
        spatial = tuple(range(2, 2 + self.n_dim))
        centre = self.conv_function(x, self.weight.sum(dim=spatial, keepdim=True), groups=self.groups)
        return (self.conv(x) - centre) / grid_width
