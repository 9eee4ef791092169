"""Attention kernel integral on the engine: AttentionKernelIntegral and its rotary embedding RotaryEmbedding2D.

Same constructors, attributes, forward signature, errors and ``state_dict()`` keys as
neuralop/layers/attention_kernel_integral.py and the RotaryEmbedding2D of neuralop/layers/embeddings.py; under one
``torch.manual_seed`` the parameters are the reference's bit for bit.  The four projections stay F.linear; everything
between them -- head split, the two norms, the rotary embedding of q and k, K^T V, q (K^T V), the quadrature weight and
the merge of the heads -- is one autograd node, engine.AttnIntegralFn, over sc_attn_forward / sc_attn_backward
(sc_kernels_attn.h), which keeps q, k, v and the (B, H, D, D) product and recomputes the rest on the way back.

Reproduced as the reference runs, not as it reads:
  * ``k_norm`` / ``v_norm`` are InstanceNorm1d modules applied to a [B H, N, D] view, where torch takes N for the
    channels and D for the length: a layer norm over the D head channels of every point (biased variance, eps 1e-5);
  * ``weights`` is multiplied by QUERY row (the reference's broadcast), although its docstring says source;
  * n_qry != n_src fails in the final view, and a 1-d rotary embedding with batch > 1 fails in a repeat.
The engine route takes fp32 device tensors, associative=True, n_qry == n_src, no rotary module or one with the
reference's inv_freq / min_freq / scale and an inv_freq of the length the position dimension calls for, batch 1 for the
1-d embedding, and positions and weights that need no gradient.  Everything else -- float64, CPU tensors,
associative=False, return_kernel, a foreign embedding module -- is the reference's formula in torch.
"""
import contextlib
import math

import torch
from torch import nn

from . import blocks, engine

ROUTES = ("auto", "engine", "torch")
_ROUTE = "auto"


@contextlib.contextmanager
def route(name):
    """Inside the block every AttentionKernelIntegral takes this route: "engine" (ValueError at a call that is not
    eligible), "torch" (the reference's formula) or "auto" (the engine wherever the call is eligible)."""
    global _ROUTE
    if name not in ROUTES:
        raise ValueError(f"AttentionKernelIntegral: route must be one of {ROUTES}, got {name!r}")
    saved, _ROUTE = _ROUTE, name
    try:
        yield
    finally:
        _ROUTE = saved


def _rotate_half(x):
    x1, x2 = x.reshape(*x.shape[:-1], 2, -1).unbind(dim=-2)
    return torch.cat((-x2, x1), dim=-1)


def _apply_rotary(t, freqs):
    return (t * freqs.cos()) + (_rotate_half(t) * freqs.sin())


class RotaryEmbedding2D(nn.Module):
    """Rotary positional embedding (https://arxiv.org/abs/2104.09864): forward gives the angles of one coordinate,
    the two static methods rotate features by them.  ``dim`` is the number of channels one coordinate rotates."""

    def __init__(self, dim, min_freq=1 / 64, scale=1.0):
        super().__init__()
        inv_freq = 1.0 / (10000 ** (torch.arange(0, dim, 2).float() / dim))
        self.min_freq = min_freq
        self.scale = scale
        self.register_buffer("inv_freq", inv_freq, persistent=False)
        self.out_channels = 2

    def forward(self, coordinates):
        """coordinates [batch, n] -> angles [batch, n, dim]"""
        coordinates = coordinates * (self.scale / self.min_freq)
        freqs = torch.einsum("... i , j -> ... i j", coordinates, self.inv_freq)
        return torch.cat((freqs, freqs), dim=-1)

    @staticmethod
    def apply_1d_rotary_pos_emb(t, freqs):
        return _apply_rotary(t, freqs)

    @staticmethod
    def apply_2d_rotary_pos_emb(t, freqs_x, freqs_y):
        d = t.shape[-1]
        return torch.cat((_apply_rotary(t[..., : d // 2], freqs_x), _apply_rotary(t[..., d // 2:], freqs_y)), dim=-1)


class AttentionKernelIntegral(nn.Module):
    """u(x_i) = sum_j (q(x_i) . k(y_j)) v(y_j) w: the kernel integral with a linear-attention kernel, self-attention
    (one input function) or cross-attention (``u_qry`` / ``pos_qry`` given).

    Parameters: in_channels, out_channels, n_heads, head_n_channels (channels of a head), project_query (False: the
    query function is used as it comes, for cross-attention)."""

    def __init__(self, in_channels, out_channels, n_heads, head_n_channels, project_query=True):
        super().__init__()
        self.n_heads = n_heads
        self.head_n_channels = head_n_channels
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.project_query = project_query
        width = head_n_channels * n_heads
        self.to_q = nn.Linear(in_channels, width, bias=False) if project_query else nn.Identity()
        self.to_k = nn.Linear(in_channels, width, bias=False)
        self.k_norm = nn.InstanceNorm1d(head_n_channels, affine=False)
        self.v_norm = nn.InstanceNorm1d(head_n_channels, affine=False)
        self.to_v = nn.Linear(in_channels, width, bias=False)
        self.to_out = nn.Linear(width, out_channels) if width != out_channels else nn.Identity()
        self.init_gain = 1 / math.sqrt(head_n_channels)
        self.diagonal_weight = self.init_gain
        self.initialize_qkv_weights()

    def init_weight(self, weight, init_fn):
        """every head's block of the projection by init_fn with the small gain, plus diagonal_weight I where a head has
        as many channels as the input"""
        d = self.head_n_channels
        for param in weight.parameters():
            if param.ndim > 1:
                for h in range(self.n_heads):
                    init_fn(param[h * d:(h + 1) * d, :], gain=self.init_gain)
                    if d == self.in_channels:
                        eye = torch.diag(torch.ones(param.size(-1), dtype=torch.float32))
                        param.data[h * d:(h + 1) * d, :] += self.diagonal_weight * eye

    def initialize_qkv_weights(self):
        """small-gain Xavier blocks with a diagonal bias (Table 8 of https://arxiv.org/pdf/2105.14995.pdf)"""
        if self.project_query:
            self.init_weight(self.to_q, nn.init.xavier_uniform_)
        self.init_weight(self.to_k, nn.init.xavier_uniform_)
        self.init_weight(self.to_v, nn.init.xavier_uniform_)

    def normalize_wrt_domain(self, u, norm_fn):
        """[B, H, N, D] through norm_fn on the [B H, N, D] view"""
        batch_size = u.shape[0]
        u = norm_fn(u.view(batch_size * self.n_heads, -1, self.head_n_channels))
        return u.view(batch_size, self.n_heads, -1, self.head_n_channels)

    # ---- route ---------------------------------------------------------------------------------------------------
    def _rotary_kind(self, module, pos_dim):
        """0 without a module, the position dimension where the module is the reference's rotary embedding with an
        inv_freq of the length the kernels index, None for anything else"""
        if module is None:
            return 0
        inv_freq = getattr(module, "inv_freq", None)
        scale, min_freq = getattr(module, "scale", None), getattr(module, "min_freq", None)
        if not torch.is_tensor(inv_freq) or not all(isinstance(s, (int, float)) and not isinstance(s, bool)
                                                      for s in (scale, min_freq)) or min_freq == 0:
            return None
        if type(module).__name__ != "RotaryEmbedding2D" or pos_dim not in (1, 2):
            return None
        d = self.head_n_channels
        if d % (2 * pos_dim) or inv_freq.dtype != torch.float32 or inv_freq.numel() != d // (2 * pos_dim):
            return None
        return pos_dim

    def on_engine(self, u_src, pos_src, positional_embedding_module=None, u_qry=None, pos_qry=None, weights=None,
                  associative=True, return_kernel=False):
        """True where forward(...) with these arguments runs the engine's kernels (module docstring)"""
        if _ROUTE == "torch" or not associative or return_kernel:
            return False
        qry = u_src if u_qry is None else u_qry
        pq = pos_src if pos_qry is None else pos_qry
        d = self.head_n_channels
        if u_src.dim() != 3 or qry.dim() != 3 or pos_src.dim() != 3 or pq.dim() != 3:
            return False
        tensors = [u_src, qry, pos_src, pq] + ([] if weights is None else [weights]) + \
            [p for p in self.parameters()]
        if any(t.dtype != torch.float32 for t in tensors) or not all(blocks._on_engine(t) for t in tensors):
            return False
        if qry.shape[1] != u_src.shape[1] or qry.shape[0] != u_src.shape[0] or d % 2 or not 2 <= d <= 128:
            return False
        if not self.project_query and qry.shape[2] != d * self.n_heads:
            return False
        kind = self._rotary_kind(positional_embedding_module, pos_src.shape[-1])
        if kind is None or (kind == 1 and u_src.shape[0] != 1):
            return False
        if kind and (pos_src.shape[:2] != u_src.shape[:2] or pq.shape[:2] != qry.shape[:2]
                     or pq.shape[-1] != pos_src.shape[-1]
                     or not blocks._on_engine(positional_embedding_module.inv_freq)):
            return False
        if pos_src.requires_grad or pq.requires_grad or (weights is not None and weights.requires_grad):
            return False
        if weights is not None and weights.numel() != u_src.shape[0] * u_src.shape[1]:
            return False
        return True

    # ---- forward -------------------------------------------------------------------------------------------------
    def forward(self, u_src, pos_src, positional_embedding_module=None, u_qry=None, pos_qry=None, weights=None,
                associative=True, return_kernel=False):
        """u_src [B, n_src, C] (keys and values), pos_src [B, n_src, pos_dim], positional_embedding_module for q / k,
        u_qry [B, n_qry, C] and pos_qry [B, n_qry, pos_dim] for cross-attention, weights [B, n] quadrature weights
        (1 / n_src without), associative: q (K^T V) instead of (q K^T) V, return_kernel: also the N x N kernel matrix
        (non-associative only).  Returns u on the query points."""
        if u_qry is None:
            if pos_qry is not None:
                raise ValueError('Query coordinates are provided but query function is not provided')
        else:
            if pos_qry is None:
                raise ValueError('Query coordinates are required if query function is provided')
        if return_kernel and associative:
            raise ValueError("Cannot get kernel matrix when associative is set to True")
        args = (u_src, pos_src, positional_embedding_module, u_qry, pos_qry, weights, associative, return_kernel)
        if not self.on_engine(*args):
            if _ROUTE == "engine":
                raise ValueError("AttentionKernelIntegral: route 'engine', but this call is not eligible for the engine "
                                 "(see on_engine)")
            return self._forward_torch(*args)
        qry = u_src if u_qry is None else u_qry
        pq = pos_src if pos_qry is None else pos_qry
        q, k, v = self.to_q(qry), self.to_k(u_src), self.to_v(u_src)
        kind = self._rotary_kind(positional_embedding_module, pos_src.shape[-1])
        inv_freq, rot_scale = None, 1.0
        if kind:
            inv_freq = positional_embedding_module.inv_freq
            rot_scale = positional_embedding_module.scale / positional_embedding_module.min_freq
        w = None if weights is None else weights.reshape(u_src.shape[0], u_src.shape[1])
        u = engine.AttnIntegralFn.apply(q, k, v, pos_src.detach() if kind else None, pq.detach() if kind else None,
                                        inv_freq, float(rot_scale), None if w is None else w.detach(), self.n_heads, kind)
        return self.to_out(u)

    def _forward_torch(self, u_src, pos_src, positional_embedding_module, u_qry, pos_qry, weights, associative,
                       return_kernel):
        """the reference's chain of torch calls, its failures included"""
        emb, heads, d = positional_embedding_module, self.n_heads, self.head_n_channels
        if u_qry is None:
            u_qry = u_src
        batch_size, num_grid_points = u_src.shape[:2]
        pos_dim = pos_src.shape[-1]

        def split(t):
            return t.view(batch_size, -1, heads, d).permute(0, 2, 1, 3).contiguous()

        q, k, v = split(self.to_q(u_qry)), split(self.to_k(u_src)), split(self.to_v(u_src))
        k = self.normalize_wrt_domain(k, self.k_norm)
        v = self.normalize_wrt_domain(v, self.v_norm)
        if emb is not None:
            if pos_dim == 2:
                def angles(pos):
                    return [emb.forward(pos[..., a]).unsqueeze(1).repeat([1, heads, 1, 1]) for a in (0, 1)]

                k_f = angles(pos_src)
                q_f = k_f if pos_qry is None else angles(pos_qry)
                q = emb.apply_2d_rotary_pos_emb(q, *q_f)
                k = emb.apply_2d_rotary_pos_emb(k, *k_f)
            elif pos_dim == 1:
                def angles(pos):
                    return emb.forward(pos[..., 0]).unsqueeze(1).repeat([batch_size, heads, 1, 1])

                k_f = angles(pos_src)
                q_f = k_f if pos_qry is None else angles(pos_qry)
                q = emb.apply_1d_rotary_pos_emb(q, q_f)
                k = emb.apply_1d_rotary_pos_emb(k, k_f)
            else:
                raise ValueError('Currently doesnt support relative embedding >= 3 dimensions')
        w = weights.view(batch_size, 1, num_grid_points, 1) if weights is not None else 1.0 / num_grid_points
        if associative:
            u = torch.matmul(q, torch.matmul(k.transpose(-1, -2), v)) * w
        else:
            kxy = torch.matmul(q, k.transpose(-1, -2))
            u = torch.matmul(kxy, v) * w
        u = u.permute(0, 2, 1, 3).contiguous().view(batch_size, num_grid_points, heads * d)
        u = self.to_out(u)
        if return_kernel:
            return u, kxy
        return u
