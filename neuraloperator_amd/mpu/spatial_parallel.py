"""Spatially decomposed ("pencil") SpectralConv: ONE sample spans the model-parallel group.

SURVEY.md section 8, "next" row f3: for B < P, or for single samples too large for one GPU (1024^2, 128^3+), the
batch cannot be sharded -- the grid is.  New functionality on the reference's mpu API shape (the reference
only has the unused building blocks, neuralop/mpu/helpers.py:28-99).  Layout per rank p of P:

    activations   row-sharded      x_p   (B, Cin, d1/P, d2..dN)         rows [p d1/P, (p+1) d1/P) of dim 1
    weights       column-sharded   W_p   (Cin, Cout, k1, k2p/P, k3..kN)  second mode dim, padded to k2p = P ceil(k2/P)

    x_p --pruned rFFT over d2..dN (local rows)--> (B, Cin, d1/P, k2, ..)
        --pad k2 -> k2p, all-to-all (split k2p, cat rows)--> (B, Cin, d1, k2p/P, ..)
        --pruned complex DFT over d1 (centred rows)--> (B, Cin, k1, k2p/P, ..)
        --contract with W_p--> (B, Cout, k1, k2p/P, ..)
        --zero-padded inverse DFT over d1--> (B, Cout, d1, k2p/P, ..)
        --all-to-all (split rows, cat k2p), drop the padding--> (B, Cout, d1/P, k2, ..)
        --zero-padded C2R over d2..dN (+ bias)--> y_p (B, Cout, d1/P, d2..dN)

Round 5: factorized weights (Tucker / CP / TT: the factors are replicated over the group, each rank reconstructs the
dense block of ITS mode columns only -- `weight[:, :, :, lo:hi].to_tensor()`, neuraloperator_amd/factorized.py -- and
contracts it on the engine; the factor gradients are summed over the group by `reduce_replicated_grads`) and a change
of resolution (`forward(x, output_shape)` / `resolution_scaling_factor`: the two inverse stages run to the output grid,
whose first dim is sharded the same way).

Round 6: runtime ``n_modes`` (<= the constructed ones: the used centred sub-block of the stored weight, modes.kept_block --
the used columns keep their place in the padded column layout, so the shard ownership never moves), grids smaller than
the modes, ``complex_data=True`` (complex-to-complex local transforms, modes.kept_block_complex and the reference's
last-dim rule, modes.analysis_freqs), ``separable=True`` (one (C, modes) weight, spectral_convolution.py:49-52) and a change of
resolution along EVERY dim (the synthesis maps of
modes.synthesis_freqs on the local transform and on the axis pass).

The skip path's resample, ``transform(x, output_shape)`` (resample.py:7-71, what FNOBlocks calls on both skips of
every block, fno_block.py:377-392), works on the row shards too, so the layer runs inside FNOBlocks / FNO with a
``resolution_scaling_factor`` or ``FNO.forward(x, output_shape=...)``.  2-d: bicubic interpolation (:49-52) -- each
rank's output rows read a contiguous range of global input rows (its own plus at most a few of its neighbours', found
with the kernel's own fp32 index arithmetic, ``bicubic_source_rows``); ``mappings.exchange_rows`` moves exactly those
rows (gradients of halo rows go back to their owners) and the engine's ``interpolate_rows`` stage
(include/sc_engine.h, sc_bicubic_rows_forward) interpolates them.  3-d and up: the spectral resample (:54-66) as the
forward pipeline above without the contraction (modes.resample_block's maps).  ``complex_data=True`` is not available
on the skip path.

Every local stage is an engine transform over fewer dims (a (N-1)-d real plan with the local rows folded into the
channel count, and a 1-d complex plan with an explicit centred frequency map -- include/sc_engine.h,
sc_plan_desc.freq); the separable N-d transform of spectral_convolution.py:443-449 / :531-559 is the product of
the two.  One all-to-all each way moves the truncated spectrum only (k2/d2 of the data); the backward is the
same pipeline mirrored.  Each rank sees the whole batch for its mode columns: gW needs no all-reduce; the bias
gradient is summed over the group (every rank saw different rows).
"""
import numpy as np
import torch
from torch import nn

from ..modes import analysis_freqs, halve_last_mode, kept_block, kept_block_complex, resample_block, synthesis_freqs
from ..spectral_conv import BaseSpectralConv
from . import comm
from .mappings import all_to_all, exchange_rows


def bicubic_source_rows(h_in, h_out, P):
    """[(lo, hi)] per rank: the global input rows the taps of rank p's output rows [p h_out / P, (p + 1) h_out / P) of
    a bicubic align_corners resample read -- ATen's fp32 index arithmetic, exactly as the kernel evaluates it
    (include/sc_engine.h, sc_bicubic_rows_forward): floor(scale dst) - 1 .. + 2, clamped to the global grid."""
    scale = np.float32(h_in - 1) / np.float32(h_out - 1) if h_out > 1 else np.float32(0)
    rows = h_out // P

    def fl(y):
        return int(np.floor(np.float32(scale) * np.float32(y)))

    return [(max(fl(p * rows) - 1, 0), min(fl((p + 1) * rows - 1) + 2, h_in - 1) + 1) for p in range(P)]


def centred_rows(k, n):
    """FFT index on an n-point grid of kept row r: signed frequency r - k//2 (spectral_convolution.py:502-512)."""
    return [(r - k // 2) % n for r in range(k)]


class SpatialParallelSpectralConv(BaseSpectralConv):
    """SpectralConv on a grid whose FIRST spatial dim is sharded across the model-parallel group.

    Constructor arguments follow SpectralConv; ``n_modes`` is fixed at construction.  Dense weights are sharded by
    columns of the second mode dim; Tucker / CP / TT weights are replicated as factors (round 5).  ``ops`` (tests only)
    replaces the local stages (forward_transform / inverse_transform / contract / forward_axis / inverse_axis)."""

    def __init__(self, in_channels, out_channels, n_modes, bias=True, init_std="auto",
                 fft_norm="forward", device=None, engine_flags=0, group=None, ops=None, factorization=None, rank=0.5,
                 fixed_rank_modes=None, resolution_scaling_factor=None, fno_block_precision="full", **unused):
        super().__init__(device=device)
        if fno_block_precision not in ("full", "half", "mixed"):
            raise ValueError(f"fno_block_precision={fno_block_precision!r}: expected full, half or mixed")
        self.fno_block_precision = fno_block_precision
        self.separable = bool(unused.get("separable", False))          # spectral_convolution.py:123-131, 49-52
        if self.separable and in_channels != out_channels:
            raise ValueError("To use separable Fourier Conv, in_channels must be equal to out_channels, "
                             f"but got in_channels={in_channels} and out_channels={out_channels}")
        self.complex_data = bool(unused.get("complex_data", False))
        fac = (factorization or "dense").lower()
        if fac not in ("dense", "tucker", "cp", "tt"):
            raise NotImplementedError("spatially decomposed layer: dense, Tucker, CP or TT weights")
        if fft_norm != "forward":
            raise NotImplementedError("spatially decomposed layer: fft_norm='forward' (the reference default)")
        self.in_channels, self.out_channels = in_channels, out_channels
        self._n_modes = halve_last_mode(n_modes, self.complex_data)
        self.max_n_modes = list(self._n_modes)
        self.order = len(self._n_modes)
        if self.order < 2:
            raise NotImplementedError("a spatial decomposition needs >= 2 spatial dims (dim 0 is sharded)")
        # spectral_convolution.py:338-347 (validate_scaling_factor): one factor per spatial dim
        if resolution_scaling_factor is not None and not isinstance(resolution_scaling_factor, (list, tuple)):
            resolution_scaling_factor = [float(resolution_scaling_factor)] * self.order
        self.resolution_scaling_factor = resolution_scaling_factor
        self.fft_norm = fft_norm
        self.factorization = fac
        self.group = group
        self.P = comm.get_model_parallel_size() if group is None else torch.distributed.get_world_size(group)
        self.rank = comm.get_model_parallel_rank() if group is None else torch.distributed.get_rank(group)
        k2 = self.max_n_modes[1]
        self.k2_pad = -(-k2 // self.P) * self.P                      # columns after padding
        self.k2_loc = self.k2_pad // self.P                          # columns this rank contracts
        if init_std == "auto":
            init_std = (2 / (in_channels + out_channels)) ** 0.5
        lo = self.rank * self.k2_loc
        lead = (in_channels,) if self.separable else (in_channels, out_channels)       # (C, modes) when separable
        self._md = len(lead)                                         # index of the first mode dim of the weight
        if fac == "dense":
            w = torch.empty(*lead, self._n_modes[0], self.k2_loc, *self._n_modes[2:], dtype=torch.cfloat, device=device)
            w.normal_(0, init_std)
            if lo + self.k2_loc > k2:                                # inert padding columns of the last rank(s)
                with torch.no_grad():
                    w.narrow(self._md + 1, max(k2 - lo, 0), self.k2_loc - max(k2 - lo, 0)).zero_()
            self.weight = nn.Parameter(w)
            self.weight.mode_sharded = True
        else:
            # the whole factorized weight on every rank (a Tucker weight of rank 0.1 is 1 / 35 of the dense one); the
            # per-rank random init is made identical by sync_replicated_parameters()
            from ..factorized import SpectralWeight
            self.weight = SpectralWeight.new((*lead, *self._n_modes), rank=rank, factorization=fac,
                                             fixed_rank_modes=fixed_rank_modes, device=device)
            self.weight.normal_(0, init_std)
        self.bias = nn.Parameter(init_std * torch.randn(out_channels, *(1,) * self.order, device=device)) \
            if bias else None
        if ops is None:
            from ..engine import EngineOps, SC_PLAN_COMPLEX
            ops = EngineOps(fft_norm, engine_flags | (SC_PLAN_COMPLEX if self.complex_data else 0))
        self.ops = ops

    def _local_weight(self, kept=None, w_start=None):
        """(Cin, Cout, k1', k2p / P, k3', ..) -- (C, k1', k2p / P, ..) when separable -- dense block of this rank's mode
        columns (zero columns past k2) restricted to the used centred sub-block of every UNSHARDED mode dim (rows
        w_start[d] .. + kept[d], modes.kept_block)"""
        mx, md = self.max_n_modes, self._md
        if kept is None:
            kept, w_start = list(mx), [0] * self.order
        sub = [slice(None)] * md + [slice(s0, s0 + k) for s0, k in zip(w_start, kept)]
        if self.factorization == "dense":
            sub[md + 1] = slice(None)
            whole = all(k == m for d, (k, m) in enumerate(zip(kept, mx)) if d != 1)
            return self.weight if whole else self.weight[tuple(sub)]
        k2 = mx[1]
        lo = self.rank * self.k2_loc
        hi = min(lo + self.k2_loc, k2)
        shape = ([self.in_channels] if self.separable else [self.in_channels, self.out_channels]) + list(kept)
        shape[md + 1] = self.k2_loc
        if hi <= lo:                                                   # a rank that holds padding only
            return torch.zeros(shape, dtype=torch.cfloat, device=next(self.weight.parameters()).device)   # (bias=False: ADVICE r5)
        sub[md + 1] = slice(lo, hi)
        w = self.weight[tuple(sub)].to_tensor()
        return _pad_dim(w, md + 1, self.k2_loc - (hi - lo)) if hi - lo != self.k2_loc else w

    def replicated_parameters(self):
        """parameters every rank holds a full copy of: the bias and the factors of a factorized weight"""
        ps = [] if self.bias is None else [self.bias]
        if self.factorization != "dense":
            ps += list(self.weight.parameters())
        return ps

    @property
    def n_modes(self):
        return self._n_modes

    @n_modes.setter
    def n_modes(self, value):
        # spectral_convolution.py:400-415; the shard layout belongs to max_n_modes and does not move
        nm = halve_last_mode(value, self.complex_data)
        if len(nm) != self.order or any(n > m for n, m in zip(nm, self.max_n_modes)) or any(n < 1 for n in nm):
            raise ValueError(f"n_modes {list(value)} must have {self.order} entries within the constructed "
                             f"max_n_modes {self.max_n_modes}")
        self._n_modes = nm

    def transform(self, x, output_shape=None):
        """The skip path's resample (resample(x, 1.0, spatial dims, output_shape), resample.py:7-71) on this rank's rows:
        ``output_shape`` is the FULL output grid, as in ``forward``; this rank returns its rows of the resampled grid.
        2-d: bicubic interpolation (:49-52) on the rows of the shard plus the halo rows its output rows read
        (mappings.exchange_rows, then the engine's interpolate_rows); 3-d and up: the spectral resample (:54-66) as
        this layer's forward pipeline without the contraction."""
        in_grid = [x.shape[2] * self.P] + list(x.shape[3:])
        out_grid = self._out_grid(in_grid, output_shape)
        if out_grid == in_grid:
            return x
        if self.complex_data:
            raise NotImplementedError("complex_data=True: the skip path's resample of complex data is not available "
                                      "on the spatially decomposed layer")
        if self.order == 2:
            return self._resample_bicubic(x, in_grid, out_grid)
        return self._resample_spectral(x, in_grid, out_grid)

    def _resample_bicubic(self, x, in_grid, out_grid):
        ranges = bicubic_source_rows(in_grid[0], out_grid[0], self.P)
        xh = exchange_rows(x, 2, ranges, group=self.group)                     # (B, C, rows of my range, W)
        h_out = out_grid[0] // self.P
        return self.ops.interpolate_rows(xh, in_grid, out_grid, ranges[self.rank][0], self.rank * h_out, h_out)

    def _resample_spectral(self, x, in_grid, out_grid):
        b, c, h_loc = x.shape[:3]
        kept, fa, fs = resample_block(in_grid, out_grid)
        d1, d1_o, h_out, rest_o = in_grid[0], out_grid[0], out_grid[0] // self.P, out_grid[1:]
        # 1. pruned transform over d2..dN on the local rows
        xh = self.ops.forward_transform(x.float().reshape(b, c * h_loc, *in_grid[1:]), kept[1:], fa[1:])
        xh = xh.reshape(b, c, h_loc, *kept[1:])
        # 2. + 3. pad the second kept dim to a multiple of P, all-to-all: every row of this rank's columns
        k2 = kept[1]
        k2p = -(-k2 // self.P) * self.P
        xh = _place_dim(xh, 3, 0, k2p)
        xh = all_to_all(xh, split_dim=3, cat_dim=2, group=self.group)          # (B, C, d1, k2p/P, ..)
        # 4. + 5. the sharded dim: kept signed rows of the old grid onto the same signed rows of the new one
        xt = xh.movedim(2, -1).contiguous()
        lead = xt.shape[:-1]
        xa = self.ops.forward_axis(xt.reshape(b, -1, d1), kept[0], fa[0])
        ya = self.ops.inverse_axis(xa, d1_o, fs[0])
        ya = ya.reshape(*lead, d1_o).movedim(-1, 2).contiguous()               # (B, C, d1', k2p/P, ..)
        # 6. all-to-all back, drop the padding
        ya = all_to_all(ya, split_dim=2, cat_dim=3, group=self.group)          # (B, C, d1'/P, k2p, ..)
        if k2p != k2:
            ya = ya.narrow(3, 0, k2)
        # 7. zero-padded inverse transform over d2..dN to the new grid
        ya = ya.reshape(b, c * h_out, *kept[1:]).contiguous()
        return self.ops.inverse_transform(ya, None, rest_o, list(fs[1:])).reshape(b, c, h_out, *rest_o)

    def _out_grid(self, in_grid, output_shape):
        """the full output grid (spectral_convolution.py:520-529: output_shape, else the scaled input grid)"""
        if output_shape is not None:
            out = [int(v) for v in output_shape]
        elif self.resolution_scaling_factor is not None:
            out = [round(n * f) for n, f in zip(in_grid, self.resolution_scaling_factor)]
        else:
            return list(in_grid)
        if len(out) != len(in_grid) or out[0] % self.P:
            raise ValueError(f"output grid {out}: {len(in_grid)} dims, the first divisible by the group size {self.P}")
        return out

    def forward(self, x, output_shape=None):
        """``output_shape``: the FULL output grid (all ranks pass the same one); this rank returns its rows of it.

        ``fno_block_precision`` "half" / "mixed" follows SpectralConv.forward: on an unchanged grid with a not-separable
        weight, x rounded to float16 ("half"), the SC_GEMM_F16 contraction of this rank's mode columns and the inverse
        transform rounded to float16 before the bias (none: a float16 result) -- SpectralConv._forward_half's cast
        points; a separable weight or a change of grid: fp32 arithmetic, the same output dtype.  The two exchanges stay
        fp32: they carry half-transformed data, not float16 values."""
        if x.ndim != self.order + 2:
            raise ValueError(f"expected a (B, C, {self.order} spatial dims) input, got {tuple(x.shape)}")
        if x.is_complex() != self.complex_data:
            raise ValueError("complex_data=True takes complex inputs (and only those)")
        if self.fno_block_precision in ("half", "mixed") and not self.complex_data:
            x = x.float()
            in_grid = [x.shape[2] * self.P] + list(x.shape[3:])
            if not self.separable and self._out_grid(in_grid, output_shape) == in_grid:
                return self._forward(x, output_shape, half=True)
            y = self._forward(x, output_shape)
            return y if self.bias is not None else y.half()      # half + fp32 bias promotes to fp32 upstream
        return self._forward(x, output_shape)

    def _forward(self, x, output_shape, half=False):
        cplx = self.complex_data
        b, c, h_loc = x.shape[:3]
        rest = list(x.shape[3:])
        d1 = h_loc * self.P
        in_grid = [d1] + rest
        kept, w_start = (kept_block_complex if cplx else kept_block)(in_grid, self._n_modes, self.max_n_modes)
        k1, k2, c0 = kept[0], kept[1], w_start[1]
        co = self.out_channels
        out_grid = self._out_grid(in_grid, output_shape)
        # which FFT index each kept row reads / lands on (None = the default centred / plain maps; a synthesis entry
        # None = the row falls off a coarser output grid and is dropped: spectral_convolution.py:524-559)
        fa = analysis_freqs(in_grid, kept, cplx)
        fs, real_col = synthesis_freqs(in_grid, out_grid, kept, cplx)
        d1_o, rest_o, h_out = out_grid[0], out_grid[1:], out_grid[0] // self.P
        if half and self.fno_block_precision == "half":
            from .. import engine
            x = engine.round_f16(x)                                                     # spectral_convolution.py:436-437
        # 1. local rows: pruned transform over d2..dN (rows folded into the channel count)
        xr = x.reshape(b, c * h_loc, *rest)
        xh = self.ops.forward_transform(xr, kept[1:]) if fa is None else self.ops.forward_transform(xr, kept[1:], fa[1:])
        xh = xh.reshape(b, c, h_loc, *kept[1:])
        # 2. exchange: every rank gets ALL rows of its k2p / P columns; the used columns sit at their place in the
        #    stored weight's (padded) column layout
        xh = _place_dim(xh, 3, c0, self.k2_pad)
        xh = all_to_all(xh, split_dim=3, cat_dim=2, group=self.group)          # (B, Cin, d1, k2p/P, ..)
        # 3. pruned complex DFT over d1 (moved last: the engine's 1-d plans run over the contiguous dim)
        xt = xh.movedim(2, -1).contiguous()
        lead = xt.shape[:-1]
        rows_a = fa[0] if fa is not None and fa[0] is not None else centred_rows(k1, d1)
        xa = self.ops.forward_axis(xt.reshape(b, -1, d1), k1, rows_a)
        xa = xa.reshape(*lead, k1).movedim(-1, 2).contiguous()                   # (B, Cin, k1, k2p/P, ..)
        # 4. contraction with this rank's mode columns
        wl = self._local_weight(kept, w_start).contiguous()
        if half:                          # the complex-half contraction (SC_GEMM_F16), forward and gradients
            from .. import _lib, engine
            m = int(np.prod(xa.shape[2:]))
            yh = engine.mode_gemm(xa.reshape(b, c, m), wl.reshape(c, co, m), m,
                                  flags=_lib.SC_GEMM_F16).reshape(b, co, *xa.shape[2:])
        else:
            yh = self.ops.contract_separable(xa, wl) if self.separable else self.ops.contract(xa, wl)   # (B, Cout, k1, k2p/P, ..)
        # 5. zero-padded inverse DFT over d1 (to the OUTPUT grid's rows)
        yt = yh.movedim(2, -1).contiguous()
        lead = yt.shape[:-1]
        # (a different output grid: the reference pads / trims the UNSHIFTED spectrum at its end, ifftn(s=...) behind
        # the ifftshift, spectral_convolution.py:524-559 -- kept row r stays at FFT index (r - k1 // 2) mod d1 of the
        # INPUT grid; on a coarser grid the rows whose index falls off the end are dropped)
        rows_o = list(fs[0]) if fs is not None and fs[0] is not None else centred_rows(k1, d1)
        if any(r is None for r in rows_o):
            keep = [r for r in range(k1) if rows_o[r] is not None]
            yt = yt.index_select(-1, torch.as_tensor(keep, device=yt.device))
            rows_o = [rows_o[r] for r in keep]
        ya = self.ops.inverse_axis(yt.reshape(b, -1, len(rows_o)), d1_o, rows_o)
        ya = ya.reshape(*lead, d1_o).movedim(-1, 2).contiguous()                 # (B, Cout, d1', k2p/P, ..)
        # 6. exchange back: local rows, all columns; keep the used ones
        ya = all_to_all(ya, split_dim=2, cat_dim=3, group=self.group)          # (B, Cout, d1/P, k2p, ..)
        if c0 or self.k2_pad != k2:
            ya = ya.narrow(3, c0, k2)
        # 7. zero-padded inverse transform over d2..dN on the local rows, bias per (channel, row) image
        ya = ya.reshape(b, co * h_out, *kept[1:]).contiguous()
        fl = None if fs is None else list(fs[1:])
        if cplx:                          # a real bias added to a complex field: elementwise glue (:567-568)
            y = self.ops.inverse_transform(ya, None, rest_o, fl).reshape(b, co, h_out, *rest_o)
            return y if self.bias is None else y + self.bias
        if half:                          # float16(inverse transform), then the bias (SpectralConv._forward_half)
            from .. import engine
            y = engine.round_f16(self.ops.inverse_transform(ya, None, rest_o)).reshape(b, co, h_out, *rest_o)
            return y + self.bias if self.bias is not None else y.half()
        bias = None
        if self.bias is not None:
            bias = self.bias.reshape(co, 1).expand(co, h_out).reshape(co * h_out, *(1,) * len(rest))
        if fl is None:
            y = self.ops.inverse_transform(ya, bias, rest_o)
        else:
            y = self.ops.inverse_transform(ya, bias, rest_o, fl, real_col)
        return y.reshape(b, co, h_out, *rest_o)

    # ---- helpers for the training loop -----------------------------------------------------------
    def reduce_replicated_grads(self):
        """Sum the gradients of the replicated parameters over the model-parallel group: the bias (every rank saw
        different rows) and the factors of a factorized weight (every rank contracted different mode columns)."""
        if self.P > 1:
            grp = self.group if self.group is not None else comm.get_model_parallel_group()
            for q in self.replicated_parameters():
                if q.grad is not None:
                    torch.distributed.all_reduce(torch.view_as_real(q.grad) if q.grad.is_complex() else q.grad, group=grp)

    def sync_replicated_parameters(self, src=0):
        """Broadcast the replicated parameters from group rank ``src`` (after a per-rank random init)."""
        if self.P > 1:
            grp = self.group if self.group is not None else comm.get_model_parallel_group()
            for q in self.replicated_parameters():
                t = torch.view_as_real(q.data) if q.is_complex() else q.data
                torch.distributed.broadcast(t, torch.distributed.get_global_rank(grp, src) if grp is not None else src,
                                            group=grp)

    @staticmethod
    def shard_dense_weight(full_weight, rank, world, separable=False):
        """Columns (second mode dim, zero-padded to a multiple of ``world``) of a full weight that ``rank`` owns."""
        dim = 2 if separable else 3
        k2 = full_weight.shape[dim]
        loc = -(-k2 // world)
        w = _pad_dim(full_weight, dim, loc * world - k2) if loc * world != k2 else full_weight
        return w.narrow(dim, rank * loc, loc).contiguous()


def _place_dim(t, dim, offset, total):
    """``t`` at ``offset`` of a zero tensor with ``total`` entries along ``dim`` (autograd: a narrow of the gradient)"""
    k = t.shape[dim]
    if offset == 0 and k == total:
        return t
    parts = []
    if offset:
        parts.append(_zeros_like_dim(t, dim, offset))
    parts.append(t)
    if total - offset - k:
        parts.append(_zeros_like_dim(t, dim, total - offset - k))
    return torch.cat(parts, dim=dim)


def _zeros_like_dim(t, dim, n):
    shape = list(t.shape)
    shape[dim] = n
    return torch.zeros(shape, dtype=t.dtype, device=t.device)


def _pad_dim(t, dim, n):
    """zero-pad ``n`` entries at the end of ``dim`` (autograd: the gradient of the padding is dropped)."""
    shape = list(t.shape)
    shape[dim] = n
    return torch.cat([t, torch.zeros(shape, dtype=t.dtype, device=t.device)], dim=dim)
