"""Equidistant discrete-continuous (DISCO) convolutions on the engine: the local integral kernel of the local neural
operator (neuralop/layers/discrete_continuous_convolution.py, EquidistantDiscreteContinuousConv2d and
EquidistantDiscreteContinuousConvTranspose2d).  Constructor arguments, defaults, assertions, errors, attributes, parameter
shapes and initial scale, the non-persistent filter buffer and the state dict are the reference's; the forward pass is
one autograd node over sc_disco_forward / sc_disco_backward (engine.DiscoConvFn) instead of an einsum that
materialises the kernel followed by conv2d / conv_transpose2d.

As in the reference the forward pass pads with zeros whatever `periodic` says (padding_mode is only an attribute), and
the filter buffer is normalised over (k0 // 2) k1 + k0 % 2 of its basis functions only.

The filter basis is torch_harmonics' where that package can be imported; otherwise it is filter_basis.py's own piecewise
linear basis, which has not been compared with torch_harmonics.

The unstructured pair DiscreteContinuousConv2d / DiscreteContinuousConvTranspose2d (arbitrary point clouds, a sparse
Psi) is below the equidistant pair: Psi is built at construction in chunks of output points (no n_out x n_in tensor
exists at any time) and normalised with segment sums, and the forward pass is one autograd node over sc_dsparse_forward /
sc_dsparse_backward (engine.SparseDiscoFn) instead of a sparse COO matrix built per call, a transposed copy of the
input, torch.mm and an einsum.  Their string grids ('equidistant', 'legendre-gauss', ...) need
torch_harmonics.quadrature._precompute_grid and raise NotImplementedError where that package cannot be imported.  The
spherical DISCO classes of torch_harmonics and the LocalNO model are not provided."""
import math

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, blocks, engine
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


# ---- point clouds: a sparse Psi ----------------------------------------------------------------------------------------
PSI_ROW_BLOCK = 1024     # points of the function's second grid whose distances to every point of the first exist at once


def _precompute_grid(n, grid, periodic):
    try:
        from torch_harmonics.quadrature import _precompute_grid as real
    except ImportError:
        raise NotImplementedError(f"the string grid {grid!r} needs the torch_harmonics package "
                                  "(torch_harmonics.quadrature._precompute_grid), which cannot be imported; pass the "
                                  "grids and quadrature weights as tensors") from None
    return real(n, grid=grid, periodic=periodic)


_ATAN_PAD = 64           # elements: a multiple of every step of torch's CPU vector loops (2 x 8, 16 or 4 floats; 2 x 4, 8 doubles)
_ATAN_PIECE = 16384      # elements per call: a multiple of _ATAN_PAD, below torch's parallel grain size of 32768


def _arctan2(y, x):
    """torch.arctan2(y, x), each element by torch's vector routine: torch hands the last elements of an array (and of
    every thread's share of a long one) to the C library's scalar routine, whose last bit can differ, so that a value
    would depend on where in the array it lies and the filter matrix on the row block.  Evaluated on a flat copy padded
    to whole vectors, in pieces too short to be shared out, no element is such a leftover.

    This rests on three properties of torch's CPU kernels, none of them documented: a vector loop takes at most
    _ATAN_PAD elements a step, what is left over goes to the scalar routine, and a loop of fewer than 32768 elements
    runs on one thread.  Where one of them stops holding, values change in their last bit only and the layer stays
    correct, but the buffers may again depend on PSI_ROW_BLOCK: tests/test_disco_sparse_reference.py
    (test_row_blocks_give_the_same_bits, test_arctan2_does_not_depend_on_the_position) fails then."""
    assert _ATAN_PIECE % _ATAN_PAD == 0 and _ATAN_PIECE < 32768
    n = y.numel()
    padded = -(-n // _ATAN_PAD) * _ATAN_PAD
    yy, xx = torch.ones(padded, dtype=y.dtype), torch.ones(padded, dtype=y.dtype)
    yy[:n], xx[:n] = y.reshape(-1), x.reshape(-1)
    out = torch.empty(padded, dtype=y.dtype)
    for lo in range(0, padded, _ATAN_PIECE):
        torch.arctan2(yy[lo:lo + _ATAN_PIECE], xx[lo:lo + _ATAN_PIECE], out=out[lo:lo + _ATAN_PIECE])
    return out[:n].reshape(y.shape)


def _precompute_convolution_filter_matrix(grid_in, grid_out, kernel_shape, quadrature_weights, normalize=True,
                                          basis_type="piecewise_linear", radius_cutoff=0.01, periodic=False,
                                          transpose_normalization=False, eps=1e-9):
    """The reference's function of this name with the same element-wise expressions, evaluated PSI_ROW_BLOCK points of
    grid_out at a time: idx (3, nnz) int64 rows (basis, point of grid_out, point of grid_in) in the order argwhere gives
    on the whole n_out x n_in matrix, and vals (nnz,).  The first (k0 // 2) k1 + k0 % 2 basis functions are divided by
    their quadrature sum + eps -- per (basis, point of grid_out) with q at the point of grid_in, or, with
    transpose_normalization, per (basis, point of grid_in) with q at the point of grid_out; float64 segment sums."""
    assert len(grid_in) == 2, "grid_in must be a 2d tensor."
    assert len(grid_out) == 2, "grid_out must be a 2d tensor."
    assert grid_in.shape[0] == 2, "grid_in must be a 2d tensor."
    assert grid_out.shape[0] == 2, "grid_out must be a 2d tensor."
    n_in, n_out = grid_in.shape[-1], grid_out.shape[-1]
    grid_in = grid_in.reshape(2, 1, n_in)
    grid_out = grid_out.reshape(2, n_out, 1)
    basis = basis_class(basis_type)(kernel_shape)
    idx_parts, val_parts = [], []
    for lo in range(0, n_out, PSI_ROW_BLOCK):
        diffs = grid_in - grid_out[:, lo:lo + PSI_ROW_BLOCK]
        if periodic:
            periodic_diffs = torch.where(diffs > 0.0, diffs - 1, diffs + 1)
            diffs = torch.where(diffs.abs() < periodic_diffs.abs(), diffs, periodic_diffs)
        r = torch.sqrt(diffs[0] ** 2 + diffs[1] ** 2)
        phi = _arctan2(diffs[1], diffs[0]) + torch.pi
        idx, vals = basis.compute_support_vals(r, phi, r_cutoff=radius_cutoff)
        idx = idx.permute(1, 0).clone()
        idx[1] += lo
        idx_parts.append(idx)
        val_parts.append(vals)
    idx, vals = torch.cat(idx_parts, dim=1), torch.cat(val_parts)
    # the blocks are in ascending order of the middle index: sorting by (basis, middle, last) restores argwhere's order
    order = torch.argsort((idx[0] * n_out + idx[1]) * n_in + idx[2])
    idx, vals = idx[:, order].contiguous(), vals[order].contiguous()
    if normalize:
        if len(kernel_shape) == 1:
            kn = math.ceil(kernel_shape[0] / 2)
        else:
            kn = (kernel_shape[0] // 2) * kernel_shape[1] + kernel_shape[0] % 2
        if transpose_normalization:
            q, seg, n_seg = quadrature_weights[idx[1]].reshape(-1), idx[0] * n_in + idx[2], n_in
        else:
            q, seg, n_seg = quadrature_weights[idx[2]].reshape(-1), idx[0] * n_out + idx[1], n_out
        kernel_size = int(idx[0].max()) + 1 if idx.shape[1] else 0
        sums = torch.zeros(max(kernel_size, kn) * n_seg, dtype=torch.float64)
        sums.index_add_(0, seg, vals.double() * q.double())
        denom = (sums + eps).to(vals.dtype)[seg]
        vals = torch.where(idx[0] < kn, vals / denom, vals)
    return idx, vals


class _SparseDisco(nn.Module):
    _transposed = False

    def __init__(self, in_channels, out_channels, grid_in, grid_out, kernel_shape, basis_type="piecewise_linear",
                 n_in=None, n_out=None, quadrature_weights=None, periodic=False, groups=1, bias=True, radius_cutoff=None):
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
        self.weight = nn.Parameter(math.sqrt(1.0 / self.groupsize) *
                                   torch.randn(out_channels, self.groupsize, self.kernel_size))
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None

        if isinstance(grid_in, torch.Tensor):
            assert isinstance(quadrature_weights, torch.Tensor)
            assert not periodic
        elif isinstance(grid_in, str):
            assert n_in is not None
            assert len(n_in) == 2
            x, wx = _precompute_grid(n_in[0], grid=grid_in, periodic=periodic)
            y, wy = _precompute_grid(n_in[1], grid=grid_in, periodic=periodic)
            x, y = torch.meshgrid(torch.from_numpy(x), torch.from_numpy(y), indexing="ij")
            wx, wy = torch.meshgrid(torch.from_numpy(wx), torch.from_numpy(wy), indexing="ij")
            grid_in = torch.stack([x.reshape(-1), y.reshape(-1)])
            quadrature_weights = (wx * wy).reshape(-1)
        else:
            raise ValueError(f"Unknown grid input type of type {type(grid_in)}")
        if isinstance(grid_out, torch.Tensor):
            pass
        elif isinstance(grid_out, str):
            assert n_out is not None
            assert len(n_out) == 2
            x, wx = _precompute_grid(n_out[0], grid=grid_out, periodic=periodic)
            y, wy = _precompute_grid(n_out[1], grid=grid_out, periodic=periodic)
            x, y = torch.meshgrid(torch.from_numpy(x), torch.from_numpy(y), indexing="ij")
            grid_out = torch.stack([x.reshape(-1), y.reshape(-1)])
        else:
            raise ValueError(f"Unknown grid output type of type {type(grid_out)}")
        assert len(grid_in.shape) == 2
        assert len(grid_out.shape) == 2
        assert len(quadrature_weights.shape) == 1
        assert grid_in.shape[0] == 2
        assert grid_out.shape[0] == 2
        self.n_in = grid_in.shape[-1]
        self.n_out = grid_out.shape[-1]
        if radius_cutoff is None:
            radius_cutoff = 2 / float(math.sqrt(self.n_in if self._transposed else self.n_out) - 1)
        if radius_cutoff <= 0.0:
            raise ValueError("Error, radius_cutoff has to be positive.")
        self.register_buffer("quadrature_weights", quadrature_weights, persistent=False)

        grid_in, grid_out, qw = grid_in.detach().cpu(), grid_out.detach().cpu(), quadrature_weights.detach().cpu()
        if self._transposed:
            idx, vals = _precompute_convolution_filter_matrix(grid_out, grid_in, self.kernel_shape, qw,
                                                              basis_type=basis_type, radius_cutoff=radius_cutoff,
                                                              periodic=periodic, transpose_normalization=True)
            k, o, i = idx[0], idx[2], idx[1]
        else:
            idx, vals = _precompute_convolution_filter_matrix(grid_in, grid_out, self.kernel_shape, qw,
                                                              basis_type=basis_type, radius_cutoff=radius_cutoff,
                                                              periodic=periodic)
            k, o, i = idx[0], idx[1], idx[2]
        # the reference's matrix form: row = basis n_out + output point, column = input point
        dev = quadrature_weights.device
        self.register_buffer("psi_idx", torch.stack([k * self.n_out + o, i], dim=0).contiguous().to(dev),
                             persistent=False)
        self.register_buffer("psi_vals", vals.contiguous().to(dev), persistent=False)

        # the engine's forms: by (output point, basis) rows with ascending input points, and by input-point rows with
        # ascending (output point, basis) columns
        nnz, rows = int(vals.numel()), self.n_out * self.kernel_size
        if max(rows, self.n_in, nnz) >= 2 ** 31:
            raise ValueError(f"n_out kernel_size = {rows}, n_in = {self.n_in} and nnz = {nnz} must fit 32-bit indices")
        row = o * self.kernel_size + k
        fwd, bwd = torch.argsort(row * self.n_in + i), torch.argsort(i * rows + row)
        v32 = vals.to(torch.float32)
        for name, order, r, c, n in (("csr", fwd, row, i, rows), ("csr_t", bwd, i, row, self.n_in)):
            splits = torch.zeros(n + 1, dtype=torch.int64)
            splits[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0)
            self.register_buffer(name + "_splits", splits.to(torch.int32).to(dev), persistent=False)
            self.register_buffer(name + "_cols", c[order].to(torch.int32).contiguous().to(dev), persistent=False)
            self.register_buffer(name + "_vals", v32[order].contiguous().to(dev), persistent=False)

    def get_local_filter_matrix(self):
        """Psi as a sparse COO matrix (kernel_size n_out, n_in): row k n_out + o, column i holds the k-th basis function
        at output point o and input point i"""
        return torch.sparse_coo_tensor(self.psi_idx, self.psi_vals, size=(self.kernel_size * self.n_out, self.n_in))

    def on_engine(self, x):
        """True where forward(x) is the engine's kernels: fp32 x (B, in_channels, n_in) on a ROCm device with fp32
        parameters and buffers.  Everything else is the reference's formula in torch."""
        tensors = [x, self.weight, self.quadrature_weights, self.psi_vals, self.csr_vals, self.csr_t_vals] + \
            ([] if self.bias is None else [self.bias])
        if x.dim() != 3 or x.shape[1] != self.groupsize * self.groups or x.shape[2] != self.n_in:
            return False
        if any(t.dtype != torch.float32 for t in tensors) or any(t.device != x.device for t in tensors):
            return False
        return blocks._on_engine(x)

    def forward(self, x):
        """x (batch, in_channels, n_in) -> (batch, out_channels, n_out)"""
        if self.on_engine(x):
            return engine.SparseDiscoFn.apply(x, self.weight, self.bias, self.quadrature_weights, self.n_out, self.groups,
                                              (self.csr_splits, self.csr_cols, self.csr_vals),
                                              (self.csr_t_splits, self.csr_t_cols, self.csr_t_vals))
        dtype = torch.promote_types(torch.promote_types(x.dtype, self.psi_vals.dtype), self.weight.dtype)
        x = self.quadrature_weights.to(dtype) * x.to(dtype)
        psi = torch.sparse_coo_tensor(self.psi_idx, self.psi_vals.to(dtype), size=(self.kernel_size * self.n_out, self.n_in))
        B, C, _ = x.shape
        x = x.reshape(B * C, self.n_in).permute(1, 0).contiguous()
        x = torch.sparse.mm(psi, x)
        x = x.permute(1, 0).reshape(B, self.groups, self.groupsize, self.kernel_size, self.n_out)
        w = self.weight.to(dtype)
        out = torch.einsum("bgckx,gock->bgox", x, w.reshape(self.groups, -1, w.shape[1], w.shape[2]))
        out = out.reshape(out.shape[0], -1, out.shape[-1])
        if self.bias is not None:
            out = out + self.bias.to(dtype).reshape(1, -1, 1)
        return out


class DiscreteContinuousConv2d(_SparseDisco):
    """Discrete-continuous convolution between two point clouds of the plane (Ocampo et al., ICLR 2023; Liu-Schiaffini et
    al., ICML 2024): out[b, o, j] = sum_{c, k} weight[o, c, k] sum_i Psi[k, j, i] q[i] x[b, c, i] + bias[o].

    in_channels, out_channels : int
    grid_in, grid_out : (2, n) tensors of point coordinates, or the name of a torch_harmonics grid with n_in / n_out
    kernel_shape : int or [int, int]
    basis_type : 'piecewise_linear' (default), 'morlet', 'zernike' (the last two need torch_harmonics)
    quadrature_weights : (n_in,) tensor, required with a tensor grid_in
    periodic : default False (string grids only)
    groups : default 1;  bias : default True
    radius_cutoff : default 2 / (sqrt(n_out) - 1)
    """
    _transposed = False


class DiscreteContinuousConvTranspose2d(_SparseDisco):
    """The transposed form: Psi is evaluated with the roles of the two grids exchanged and normalised per (basis, output
    point) with the quadrature weight of the input point; radius_cutoff defaults to 2 / (sqrt(n_in) - 1).  The forward
    pass and the weight layout (out_channels, in_channels / groups, K) are those of DiscreteContinuousConv2d."""
    _transposed = True
