"""LocalNOBlocks on the engine (neuralop/layers/local_no_block.py): neural operator blocks that add a differential and a
local integral branch to the Fourier layer (Liu-Schiaffini et al., ICML 2024).  Per layer

    x -> non_linearity( norm( convs[i](x) + differential[j](x, h) + local_convs[k](x) ) + local_no_skips[i](x) )
         [ -> mlp[i](.) + channel_mlp_skips[i](x), norm, non_linearity ]

Constructor arguments, defaults, checks, warnings, attributes and module names are the reference's, so a reference
``state_dict()`` loads.  The forward pass is the post-activation path built from what the engine has: SpectralConv (with
the add + GELU epilogue of its inverse transform where no normalisation sits between the sum and the skip),
fused_linear for the 1 x 1 skips, fused_channel_mlp, FiniteDifferenceConvolution and
EquidistantDiscreteContinuousConv2d.  Normalisation (None, "group_norm", "instance_norm") runs as torch ops.

Deviations: ``preactivation=True`` raises NotImplementedError at construction -- the reference's own pre-activation path
reads an attribute (default_grid_res) that does not exist; ``norm="ada_in"`` raises NotImplementedError."""
import warnings

import torch
import torch.nn.functional as F
from torch import nn

from .blocks import fused_channel_mlp, fused_linear
from .differential_conv import FiniteDifferenceConvolution
from .discrete_continuous_convolution import EquidistantDiscreteContinuousConv2d
from .spectral_conv import SpectralConv


def _validate_scaling_factor(scaling_factor, n_dim, n_layers):
    """the per-layer form of neuralop/utils.py validate_scaling_factor: None, or one list of n_dim floats per layer"""
    if scaling_factor is None:
        return None
    if isinstance(scaling_factor, (float, int)):
        return [[float(scaling_factor)] * n_dim] * n_layers
    if isinstance(scaling_factor, list) and len(scaling_factor) > 0:
        if all(isinstance(s, (float, int)) for s in scaling_factor):
            return [[float(s)] * n_dim for s in scaling_factor]
        if all(isinstance(s, list) and all(isinstance(v, (float, int)) for v in s) for s in scaling_factor):
            return scaling_factor
    return None


class SoftGating(nn.Module):
    """x * w with w (1, channels, 1, ..): the reference's soft-gating skip"""

    def __init__(self, in_features, out_features=None, n_dim=2, bias=False):
        super().__init__()
        if out_features is not None and in_features != out_features:
            raise ValueError(f"Got in_features={in_features} and out_features={out_features}, "
                             "but these two must be the same for soft-gating")
        self.in_features, self.out_features = in_features, out_features
        self.weight = nn.Parameter(torch.ones(1, in_features, *(1,) * n_dim))
        self.bias = nn.Parameter(torch.ones(1, in_features, *(1,) * n_dim)) if bias else None

    def forward(self, x):
        return self.weight * x + self.bias if self.bias is not None else self.weight * x


class LinearSkip(nn.Module):
    """1 x 1 convolution over the channels (the reference's Flattened1dConv: the parameter lives in ``conv``), on the
    engine through fused_linear"""

    def __init__(self, in_channels, out_channels, bias=False):
        super().__init__()
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size=1, bias=bias)

    def forward(self, x):
        return fused_linear(x, self.conv.weight, self.conv.bias)


def skip_connection(in_features, out_features, n_dim=2, bias=False, skip_type="soft-gating"):
    if skip_type.lower() == "soft-gating":
        return SoftGating(in_features, out_features, n_dim=n_dim, bias=bias)
    if skip_type.lower() == "linear":
        return LinearSkip(in_features, out_features, bias=bias)
    if skip_type.lower() == "identity":
        return nn.Identity()
    raise ValueError(f"Got skip-connection type={skip_type}, expected one of {'soft-gating', 'linear', 'id'}.")


class ChannelMLP(nn.Module):
    """two 1 x 1 convolutions over the channels with the non-linearity between them (the reference's ChannelMLP with
    its default two layers: parameters in ``fcs``), on the engine through fused_channel_mlp"""

    def __init__(self, in_channels, out_channels=None, hidden_channels=None, n_dim=2, non_linearity=F.gelu, dropout=0.0):
        super().__init__()
        self.n_layers = 2
        self.in_channels = in_channels
        self.out_channels = in_channels if out_channels is None else out_channels
        self.hidden_channels = in_channels if hidden_channels is None else hidden_channels
        self.non_linearity = non_linearity
        self.dropout = nn.ModuleList([nn.Dropout(dropout) for _ in range(2)]) if dropout > 0.0 else None
        self.fcs = nn.ModuleList([nn.Conv1d(self.in_channels, self.hidden_channels, 1),
                                  nn.Conv1d(self.hidden_channels, self.out_channels, 1)])

    def fusable(self):
        return self.non_linearity is F.gelu and self.dropout is None

    def forward(self, x, skip_src=None, gate=None, activation=None):
        """mlp(x), or activation(mlp(x) + gate * skip_src) in one engine pass"""
        fc1, fc2 = self.fcs
        if self.fusable():
            return fused_channel_mlp(x, fc1.weight, fc1.bias, fc2.weight, fc2.bias, skip_src, gate, activation)
        assert skip_src is None and activation is None
        size = list(x.shape)
        h = self.non_linearity(fc1(x.reshape(*size[:2], -1)))
        h = fc2(self.dropout[0](h)) if self.dropout is not None else fc2(h)
        if self.dropout is not None:
            h = self.dropout[1](h)
        return h.reshape(size[0], self.out_channels, *size[2:])


class InstanceNorm(nn.Module):
    def __init__(self, **kwargs):
        super().__init__()
        self.kwargs = kwargs

    def forward(self, x):
        return F.instance_norm(x, **self.kwargs)


class SubModule(nn.Module):
    """one layer of a jointly parametrised LocalNOBlocks: the parameters are the main module's"""

    def __init__(self, main_module, indices):
        super().__init__()
        self.main_module = main_module
        self.indices = indices

    def forward(self, x):
        return self.main_module.forward(x, self.indices)


class LocalNOBlocks(nn.Module):
    """n_layers local neural operator layers; forward(x, index, output_shape) applies layer ``index``.

    in_channels, out_channels : int
    n_modes : int or list of int; default_in_shape : the grid the layers are built for (one entry per dimension)
    resolution_scaling_factor, n_layers, max_n_modes, use_channel_mlp, channel_mlp_dropout, channel_mlp_expansion,
    non_linearity, stabilizer, norm, norm_groups, local_no_skip, channel_mlp_skip, separable, factorization, rank,
    conv_module, fixed_rank_modes, implementation, decomposition_kwargs, fft_norm, enforce_hermitian_symmetry :
        as in the FNO blocks
    disco_layers : bool or one bool per layer (2-d only); disco_kernel_shape, radius_cutoff, domain_length, disco_groups,
        disco_bias : the local integral kernel, EquidistantDiscreteContinuousConv2d on default_in_shape
    diff_layers : bool or one bool per layer (at most 3-d); conv_padding_mode, fin_diff_kernel_size, mix_derivatives :
        the differential kernel, FiniteDifferenceConvolution
    """

    def __init__(self, in_channels, out_channels, n_modes, default_in_shape, resolution_scaling_factor=None, n_layers=1,
                 disco_layers=True, disco_kernel_shape=[2, 4], radius_cutoff=None, domain_length=[2, 2], disco_groups=1,
                 disco_bias=True, diff_layers=True, conv_padding_mode="periodic", fin_diff_kernel_size=3,
                 mix_derivatives=True, max_n_modes=None, local_no_block_precision="full", use_channel_mlp=False,
                 channel_mlp_dropout=0, channel_mlp_expansion=0.5, non_linearity=F.gelu, stabilizer=None, norm=None,
                 norm_groups=1, ada_in_features=None, preactivation=False, local_no_skip="linear",
                 channel_mlp_skip="soft-gating", separable=False, factorization=None, rank=1.0,
                 conv_module=SpectralConv, fixed_rank_modes=False, implementation="factorized",
                 decomposition_kwargs=dict(), fft_norm="forward", enforce_hermitian_symmetry=True):
        super().__init__()
        if isinstance(n_modes, int):
            n_modes = [n_modes]
        self._n_modes = n_modes
        assert len(n_modes) == len(default_in_shape), "Spatiotemporal dimensions must be consistent"
        if isinstance(disco_layers, bool):
            disco_layers = [disco_layers] * n_layers
        if isinstance(diff_layers, bool):
            diff_layers = [diff_layers] * n_layers
        if len(n_modes) > 3 and True in diff_layers:
            raise NotImplementedError("Differential convs not implemented for dimensions higher than 3.")
        if len(n_modes) != 2 and True in disco_layers:
            raise NotImplementedError("Local conv layers only implemented for dimension 2.")
        if conv_padding_mode not in ["circular", "periodic", "zeros"] and True in disco_layers:
            warnings.warn("Local conv layers only support periodic or zero padding, defaulting to zero padding for "
                          "local convs.")
        if preactivation:
            raise NotImplementedError("LocalNOBlocks(preactivation=True): only the post-activation path is provided")
        self.n_dim = len(n_modes)
        self.resolution_scaling_factor = _validate_scaling_factor(resolution_scaling_factor, self.n_dim, n_layers)
        self.max_n_modes = max_n_modes
        self.local_no_block_precision = local_no_block_precision
        self.in_channels, self.out_channels, self.n_layers = in_channels, out_channels, n_layers
        self.non_linearity, self.stabilizer = non_linearity, stabilizer
        self.rank, self.factorization, self.fixed_rank_modes = rank, factorization, fixed_rank_modes
        self.decomposition_kwargs = decomposition_kwargs
        self.local_no_skip, self.channel_mlp_skip = local_no_skip, channel_mlp_skip
        self.use_channel_mlp = use_channel_mlp
        self.channel_mlp_expansion, self.channel_mlp_dropout = channel_mlp_expansion, channel_mlp_dropout
        self.fft_norm, self.implementation, self.separable = fft_norm, implementation, separable
        self.preactivation, self.ada_in_features = preactivation, ada_in_features
        self.enforce_hermitian_symmetry = enforce_hermitian_symmetry
        self.diff_layers, self.conv_padding_mode = diff_layers, conv_padding_mode
        self.default_in_shape = default_in_shape
        self.fin_diff_kernel_size, self.mix_derivatives = fin_diff_kernel_size, mix_derivatives
        self.disco_layers, self.disco_kernel_shape = disco_layers, disco_kernel_shape
        self.radius_cutoff, self.domain_length = radius_cutoff, domain_length
        self.disco_groups, self.disco_bias = disco_groups, disco_bias
        self.periodic = self.conv_padding_mode in ["circular", "periodic"]
        assert len(diff_layers) == n_layers, \
            f"diff_layers must either provide a single bool value or a list of booleans of length n_layers, " \
            f"got {len(diff_layers)=}"
        assert len(disco_layers) == n_layers, \
            f"disco_layers must either provide a single bool value or a list of booleans of length n_layers, " \
            f"got {len(disco_layers)=}"

        hermitian = {"enforce_hermitian_symmetry": enforce_hermitian_symmetry} \
            if issubclass(conv_module, SpectralConv) else {}
        self.convs = nn.ModuleList([
            conv_module(self.in_channels, self.out_channels, self.n_modes,
                        resolution_scaling_factor=(self.resolution_scaling_factor[i]
                                                   if resolution_scaling_factor is not None else None),
                        max_n_modes=max_n_modes, rank=rank, fixed_rank_modes=fixed_rank_modes,
                        implementation=implementation, separable=separable, factorization=factorization,
                        decomposition_kwargs=decomposition_kwargs, **hermitian)
            for i in range(n_layers)])
        if local_no_skip is not None:
            self.local_no_skips = nn.ModuleList([
                skip_connection(self.in_channels, self.out_channels, skip_type=local_no_skip, n_dim=self.n_dim)
                for _ in range(n_layers)])
        else:
            self.local_no_skips = None
        self.diff_groups = 1 if mix_derivatives else in_channels
        self.differential = nn.ModuleList([
            FiniteDifferenceConvolution(self.in_channels, self.out_channels, self.n_dim, self.fin_diff_kernel_size,
                                        self.diff_groups, self.conv_padding_mode)
            for _ in range(sum(self.diff_layers))])
        self.local_convs = nn.ModuleList([
            EquidistantDiscreteContinuousConv2d(self.in_channels, self.out_channels, in_shape=self.default_in_shape,
                                                out_shape=self.default_in_shape, kernel_shape=self.disco_kernel_shape,
                                                domain_length=self.domain_length, radius_cutoff=self.radius_cutoff,
                                                periodic=self.periodic, groups=self.disco_groups, bias=self.disco_bias)
            for _ in range(sum(self.disco_layers))])
        # layer index -> index into differential / local_convs, -1 without that branch
        self.differential_idx_list = self._branch_indices(self.diff_layers)
        self.disco_idx_list = self._branch_indices(self.disco_layers)

        if use_channel_mlp:
            self.mlp = nn.ModuleList([
                ChannelMLP(in_channels=self.out_channels, hidden_channels=round(self.out_channels * channel_mlp_expansion),
                           dropout=channel_mlp_dropout, n_dim=self.n_dim)
                for _ in range(n_layers)])
            if channel_mlp_skip is not None:
                self.channel_mlp_skips = nn.ModuleList([
                    skip_connection(self.in_channels, self.out_channels, skip_type=channel_mlp_skip, n_dim=self.n_dim)
                    for _ in range(n_layers)])
            else:
                self.channel_mlp_skips = None
        else:
            self.mlp = None

        self.n_norms = 1 if self.mlp is None else 2
        if norm is None:
            self.norm = None
        elif norm == "instance_norm":
            self.norm = nn.ModuleList([InstanceNorm() for _ in range(n_layers * self.n_norms)])
        elif norm == "group_norm":
            self.norm = nn.ModuleList([nn.GroupNorm(num_groups=norm_groups, num_channels=self.out_channels)
                                       for _ in range(n_layers * self.n_norms)])
        elif norm == "ada_in":
            raise NotImplementedError("LocalNOBlocks(norm='ada_in') is not provided")
        else:
            raise ValueError(f"Got norm={norm} but expected None or one of [instance_norm, group_norm, ada_in]")

    @staticmethod
    def _branch_indices(flags):
        out, j = [], 0
        for on in flags:
            out.append(j if on else -1)
            j += 1 if on else 0
        assert max(out) == sum(flags) - 1
        return out

    def forward(self, x, index=0, output_shape=None):
        return self.forward_with_postactivation(x, index, output_shape)

    def forward_with_postactivation(self, x, index=0, output_shape=None):
        conv = self.convs[index]
        x_in = x
        skip = None
        if self.local_no_skips is not None:
            skip = conv.transform(self.local_no_skips[index](x), output_shape=output_shape)
        if self.stabilizer == "tanh":
            x = torch.tanh(x)
        local = None                                         # differential + local integral branch
        if self.differential_idx_list[index] != -1:
            h = 1 / (x.shape[-1] / self.default_in_shape[0])
            local = conv.transform(self.differential[self.differential_idx_list[index]](x, h), output_shape=output_shape)
        if self.disco_idx_list[index] != -1:
            y = conv.transform(self.local_convs[self.disco_idx_list[index]](x), output_shape=output_shape)
            local = y if local is None else local + y
        activate = (self.mlp is not None) or (index < (self.n_layers - 1))
        gelu = self.non_linearity is F.gelu
        if self.norm is None and gelu and output_shape is None and hasattr(conv, "forward_fused") and \
                getattr(conv, "resolution_scaling_factor", None) is None and (local is not None or skip is not None):
            # conv(x) + branches + skip and the activation in the inverse transform's store path
            rest = local if skip is None else (skip if local is None else local + skip)
            x = conv.forward_fused(x, rest, "gelu" if activate else None)
        else:
            x = conv(x, output_shape=output_shape)
            if local is not None:
                x = x + local
            if self.norm is not None:
                x = self.norm[self.n_norms * index](x)
            if skip is not None:
                x = x + skip
            if activate:
                x = self.non_linearity(x)
        if self.mlp is None:
            return x
        mlp, last_act = self.mlp[index], index < (self.n_layers - 1)
        mskip = None if self.channel_mlp_skips is None else self.channel_mlp_skips[index]
        same_grid = tuple(x.shape[2:]) == tuple(x_in.shape[2:])
        if isinstance(mskip, SoftGating) and mskip.bias is None and self.norm is None and gelu and mlp.fusable() and \
                same_grid:
            return mlp(x, x_in, mskip.weight, "gelu" if last_act else None)
        x = mlp(x)
        if mskip is not None:
            x = x + conv.transform(mskip(x_in), output_shape=output_shape)
        if self.norm is not None:
            x = self.norm[self.n_norms * index + 1](x)
        return self.non_linearity(x) if last_act else x

    @property
    def n_modes(self):
        return self._n_modes

    @n_modes.setter
    def n_modes(self, n_modes):
        for i in range(self.n_layers):
            self.convs[i].n_modes = n_modes
        self._n_modes = n_modes

    def get_block(self, indices):
        """a sub-block that shares its parameters with this one"""
        if self.n_layers == 1:
            raise ValueError("A single layer is parametrized, directly use the main class.")
        return SubModule(self, indices)

    def __getitem__(self, indices):
        return self.get_block(indices)
