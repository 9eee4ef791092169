"""Graph neural operator layer on the engine: NeighborSearch, segment_csr, IntegralTransform, GNOBlock.

Same constructors, forward signatures, return keys and errors as neuralop/layers/neighbor_search.py, segment_csr.py,
integral_transform.py and gno_block.py; ``state_dict()`` keys and shapes equal the reference's.  The neighbour search is
sc_radius_count / sc_radius_fill, the gather + products + segment reduction of the kernel integral one sc_csr_reduce,
and -- where the kernel MLP is a LinearChannelMLP with GELU (or a single layer) -- its first Linear is applied to points
instead of edges and sc_edge_lift forms the first hidden layer (sc_kernels_gno.h).  The remaining Linear layers run on
one of two routes (``kernel_route``): "edges", F.linear over edge-sized tensors, or "fused", engine.EdgeMlpFn -- the
whole chain in chunks of edges on sc_edge_mlp_forward / sc_edge_mlp_backward (sc_kernels_gno_mlp.h), which keeps no
tensor of E x hidden width, forward or backward.  "auto" is engine.edge_mlp_route by the shape.  fp32 on a ROCm device
only; there is no CPU path.
"""
import contextlib

import torch
import torch.nn.functional as F
from torch import nn

from . import engine

TRANSFORM_TYPES = ("linear_kernelonly", "linear", "nonlinear_kernelonly", "nonlinear")
KERNEL_ROUTES = ("auto", "edges", "fused")
_ROUTE_OVERRIDE = None


@contextlib.contextmanager
def kernel_route(name):
    """Inside the block every IntegralTransform takes this route for its kernel MLP, whatever it was built with:
    "edges", "fused" (ValueError at a layer that is not eligible) or "auto"."""
    global _ROUTE_OVERRIDE
    if name not in KERNEL_ROUTES:
        raise ValueError(f"IntegralTransform: kernel_route must be one of {KERNEL_ROUTES}, got {name!r}")
    saved, _ROUTE_OVERRIDE = _ROUTE_OVERRIDE, name
    try:
        yield
    finally:
        _ROUTE_OVERRIDE = saved


class LinearChannelMLP(nn.Module):
    """neuralop/layers/channel_mlp.py LinearChannelMLP restated: Linear layers ``fcs`` with a non-linearity between."""

    def __init__(self, layers, non_linearity=F.gelu, dropout=0.0):
        super().__init__()
        self.n_layers = len(layers) - 1
        assert self.n_layers >= 1, "Error: trying to instantiate a LinearChannelMLP with only one linear layer."
        self.in_channels, self.out_channels = layers[0], layers[-1]
        self.fcs = nn.ModuleList(nn.Linear(layers[j], layers[j + 1]) for j in range(self.n_layers))
        self.non_linearity = non_linearity
        self.dropout = nn.ModuleList([nn.Dropout(dropout) for _ in range(self.n_layers)]) if dropout > 0.0 else None

    def forward(self, x):
        for i, fc in enumerate(self.fcs):
            x = fc(x)
            if i < self.n_layers - 1:
                x = self.non_linearity(x)
            if self.dropout is not None:
                x = self.dropout[i](x)
        return x


class SinusoidalEmbedding(nn.Module):
    """neuralop/layers/embeddings.py SinusoidalEmbedding restated in torch (per point and cheap; no parameters)."""

    def __init__(self, in_channels, num_frequencies=None, embedding_type="transformer", max_positions=10000):
        super().__init__()
        allowed = ["nerf", "transformer"]
        assert embedding_type in allowed, f"Error: embedding_type expected one of {allowed}, received {embedding_type}"
        if embedding_type == "transformer":
            assert max_positions is not None, "Error: max_positions must have an int value for transformer embedding."
        self.in_channels, self.num_frequencies = in_channels, num_frequencies
        self.embedding_type, self.max_positions = embedding_type, max_positions

    @property
    def out_channels(self):
        return 2 * self.num_frequencies * self.in_channels

    def forward(self, x):
        assert x.ndim in [2, 3], f"Error: expected inputs of shape (batch, n_in, {self.in_channels}) or (n_in, channels), " \
                                 f"got inputs with ndim={x.ndim}, shape={x.shape}"
        batched = x.ndim == 3
        if not batched:
            x = x.unsqueeze(0)
        if self.embedding_type == "nerf":
            freqs = 2 ** torch.arange(0, self.num_frequencies, device=x.device) * torch.pi
        else:
            freqs = torch.arange(0, self.num_frequencies, device=x.device) / self.num_frequencies * 2
            freqs = (1 / self.max_positions) ** freqs
        ang = torch.einsum("bij, k -> bijk", x, freqs.to(x.dtype))
        out = torch.stack((ang.sin(), ang.cos()), dim=-1).reshape(x.shape[0], x.shape[1], -1)
        return out if batched else out.squeeze(0)


class NeighborSearch(nn.Module):
    """For each point of ``queries`` the indices of all points of ``data`` within ``radius``, in CSR form
    (neighbors_index int64, neighbors_row_splits int64 [m + 1], with return_norm also weights = squared distances).
    ``use_open3d`` is accepted and ignored: the search is the engine's for d = 1, 2, 3.  ``method``: "brute", "grid" (a
    uniform cell grid) or "auto" (engine.radius_route by the shape); the result is the same bytes on either."""

    def __init__(self, use_open3d=True, return_norm=False, method="auto"):
        super().__init__()
        if method not in engine.RADIUS_METHODS:
            raise ValueError(f"neighbor search: method must be one of {engine.RADIUS_METHODS}, got {method!r}")
        self.use_open3d = False
        self.return_norm = return_norm
        self.method = method

    def forward(self, data, queries, radius):
        return engine.radius_search(data, queries, radius, self.return_norm, self.method)


def segment_csr(src, indptr, reduction, use_scatter=True):
    """Sum or mean of src (E, c) / (b, E, c) over the segments indptr (m + 1,) / (b, m + 1) (the first row of a batched
    indptr is used, as in the reference).  ``use_scatter`` is accepted and ignored."""
    if reduction not in ["mean", "sum"]:
        raise ValueError("reduce must be one of 'mean', 'sum'")
    if src.ndim not in (2, 3):
        raise ValueError(f"segment_csr: src must be (E, c) or (b, E, c), got {tuple(src.shape)}")
    splits = indptr[0] if indptr.ndim == 2 else indptr
    graph = engine.CsrGraph(splits, None, 0, n_edges=src.shape[-2])
    return engine.SegmentCsrFn.apply(src, graph, reduction == "mean")


class IntegralTransform(nn.Module):
    """Integral kernel transform (GNO): (a) int k(x, y) dy, (b) int k(x, y) f(y) dy, (c) int k(x, y, f(y)) dy,
    (d) int k(x, y, f(y)) f(y) dy for transform_type linear_kernelonly / linear / nonlinear_kernelonly / nonlinear.
    ``use_torch_scatter`` is accepted and ignored.  ``kernel_route``: "edges", "fused" or "auto" (see the module's
    header); the context manager kernel_route() overrides it."""

    def __init__(self, channel_mlp=None, channel_mlp_layers=None, channel_mlp_non_linearity=F.gelu,
                 transform_type="linear", weighting_fn=None, reduction="sum", use_torch_scatter=True,
                 kernel_route="auto"):
        super().__init__()
        assert channel_mlp is not None or channel_mlp_layers is not None
        if kernel_route not in KERNEL_ROUTES:
            raise ValueError(f"IntegralTransform: kernel_route must be one of {KERNEL_ROUTES}, got {kernel_route!r}")
        self.kernel_route = kernel_route
        self.reduction = reduction
        self.transform_type = transform_type
        self.use_torch_scatter = use_torch_scatter
        if transform_type not in TRANSFORM_TYPES:
            raise ValueError(f"Got transform_type={transform_type} but expected one of "
                             "[linear_kernelonly, linear, nonlinear_kernelonly, nonlinear]")
        if channel_mlp is None:
            self.channel_mlp = LinearChannelMLP(layers=channel_mlp_layers, non_linearity=channel_mlp_non_linearity)
        else:
            self.channel_mlp = channel_mlp
        self.weighting_fn = weighting_fn

    def lift_route(self):
        """True where the first Linear runs on points (sc_edge_lift): a LinearChannelMLP without dropout whose
        non-linearity is F.gelu, or which has a single layer."""
        mlp = self.channel_mlp
        return (isinstance(mlp, LinearChannelMLP) and mlp.dropout is None
                and (mlp.n_layers == 1 or mlp.non_linearity is F.gelu))

    def fused_eligible(self):
        """True where the whole kernel MLP can run in chunks of edges (engine.EdgeMlpFn): the first layer on points, at
        least two layers, GELU between them, no width above engine.EDGE_MLP_MAX_WIDTH"""
        mlp = self.channel_mlp
        return (self.lift_route() and 2 <= mlp.n_layers <= engine.EDGE_MLP_MAX_LAYERS
                and all(fc.out_features <= engine.EDGE_MLP_MAX_WIDTH for fc in mlp.fcs))

    def _route(self, n_edges, batch):
        want = _ROUTE_OVERRIDE or self.kernel_route
        if want == "fused" and not self.fused_eligible():
            raise ValueError("IntegralTransform: kernel_route='fused' needs a LinearChannelMLP of 2 to "
                             f"{engine.EDGE_MLP_MAX_LAYERS} layers with GELU, no dropout and widths of at most "
                             f"{engine.EDGE_MLP_MAX_WIDTH}")
        if want == "auto":
            want = "edges"
            if self.fused_eligible():
                want = engine.edge_mlp_route(n_edges, batch, [fc.out_features for fc in self.channel_mlp.fcs])
        return want

    def _kernel(self, y, x, f_y, graph, nonlinear):
        mlp = self.channel_mlp
        route = self._route(graph.n_edges, f_y.shape[0] if nonlinear and f_y.ndim == 3 else 1)
        if self.lift_route():
            fc0, dy, dx = mlp.fcs[0], y.shape[-1], x.shape[-1]
            want = dy + dx + (f_y.shape[-1] if nonlinear else 0)
            if fc0.in_features != want:
                raise ValueError(f"IntegralTransform: the kernel MLP takes {fc0.in_features} channels, the inputs give {want}")
            Py = F.linear(y, fc0.weight[:, :dy])
            Px = F.linear(x, fc0.weight[:, dy:dy + dx])
            if nonlinear:
                Py = Py + F.linear(f_y, fc0.weight[:, dy + dx:])
            if route == "fused":
                later = [t for fc in mlp.fcs[1:] for t in (fc.weight, fc.bias)]
                return engine.EdgeMlpFn.apply(Py, Px, fc0.bias, graph, engine.EDGE_MLP_CHUNK_EDGES, *later)
            h = engine.EdgeLiftFn.apply(Py, Px, fc0.bias, graph, mlp.n_layers > 1)
            for i in range(1, mlp.n_layers):
                h = mlp.fcs[i](h)
                if i < mlp.n_layers - 1:
                    h = F.gelu(h)
            return h
        # any other kernel network: edge features assembled as the reference does
        agg = torch.cat([y[graph.index], torch.repeat_interleave(x, graph.splits[1:] - graph.splits[:-1], dim=0,
                                                                 output_size=graph.n_edges)], dim=-1)
        if nonlinear:
            if f_y.ndim == 3:
                agg = agg.repeat([f_y.shape[0]] + [1] * agg.ndim)
            agg = torch.cat([agg, f_y[..., graph.index, :]], dim=-1)
        return mlp(agg)

    def forward(self, y, neighbors, x=None, f_y=None, weights=None):
        if x is None:
            x = y
        if self.reduction not in ["mean", "sum"]:
            raise ValueError("reduce must be one of 'mean', 'sum'")
        graph = engine.CsrGraph(neighbors["neighbors_row_splits"], neighbors["neighbors_index"], y.shape[0])
        if graph.rows != x.shape[0]:
            raise ValueError(f"IntegralTransform: neighbors_row_splits holds {graph.rows} rows for {x.shape[0]} points x")
        if f_y is not None and (f_y.ndim not in (2, 3) or f_y.shape[-2] != y.shape[0]):
            raise ValueError(f"IntegralTransform: f_y {tuple(f_y.shape)} against {y.shape[0]} points y")
        nonlinear = f_y is not None and self.transform_type in ("nonlinear_kernelonly", "nonlinear")
        nbr_weights = neighbors.get("weights")
        if nbr_weights is None:
            nbr_weights = weights
        if nbr_weights is None and self.weighting_fn is not None:
            raise KeyError("if a weighting function is provided, your neighborhoods must contain weights.")
        mean = self.reduction == "mean"
        if nbr_weights is not None:
            if nbr_weights.requires_grad:
                raise NotImplementedError("IntegralTransform: neighbour weights that require grad are not supported")
            if self.weighting_fn is not None:
                nbr_weights = self.weighting_fn(nbr_weights)
            nbr_weights = nbr_weights.detach().reshape(-1)
            mean = False                                    # weighted layers force the sum
        k = self._kernel(y, x, f_y, graph, nonlinear)
        f_in = f_y if f_y is not None and self.transform_type != "nonlinear_kernelonly" else None
        return engine.KernelIntegralFn.apply(k, f_in, graph, nbr_weights, mean)


class GNOBlock(nn.Module):
    """Graph neural operator layer: neighbour search within ``radius``, optional sinusoidal embedding of both point
    sets, kernel integral.  ``use_torch_scatter_reduce`` / ``use_open3d_neighbor_search`` are accepted; the latter still
    asserts coord_dim == 3 as the reference does."""

    def __init__(self, in_channels, out_channels, coord_dim, radius, transform_type="linear", weighting_fn=None,
                 reduction="sum", pos_embedding_type="transformer", pos_embedding_channels=32,
                 pos_embedding_max_positions=10000, channel_mlp_layers=[128, 256, 128],
                 channel_mlp_non_linearity=F.gelu, channel_mlp=None, use_torch_scatter_reduce=True,
                 use_open3d_neighbor_search=True):
        super().__init__()
        self.in_channels, self.out_channels, self.coord_dim, self.radius = in_channels, out_channels, coord_dim, radius
        self.pos_embedding_type = pos_embedding_type
        if pos_embedding_type in ["nerf", "transformer"]:
            self.pos_embedding = SinusoidalEmbedding(in_channels=coord_dim, num_frequencies=pos_embedding_channels,
                                                     embedding_type=pos_embedding_type,
                                                     max_positions=pos_embedding_max_positions)
        else:
            self.pos_embedding = None
        if use_open3d_neighbor_search:
            assert self.coord_dim == 3, f"Error: open3d is only designed for 3d data, GNO instantiated for dim={coord_dim}"
        self.neighbor_search = NeighborSearch(use_open3d=use_open3d_neighbor_search, return_norm=weighting_fn is not None)
        if self.pos_embedding is None:
            kernel_in_dim, kernel_in_dim_str = self.coord_dim * 2, "dim(y) + dim(x)"
        else:
            kernel_in_dim, kernel_in_dim_str = self.pos_embedding.out_channels * 2, "dim(y_embed) + dim(x_embed)"
        if transform_type == "nonlinear" or transform_type == "nonlinear_kernelonly":
            kernel_in_dim += self.in_channels
            kernel_in_dim_str += " + dim(f_y)"
        if channel_mlp is not None:
            assert channel_mlp.in_channels == kernel_in_dim, \
                f"Error: expected ChannelMLP to take input with {kernel_in_dim} channels (feature channels=" \
                f"{kernel_in_dim_str}), got {channel_mlp.in_channels}."
            assert channel_mlp.out_channels == out_channels, \
                f"Error: expected ChannelMLP to have {out_channels=} but got {channel_mlp.in_channels=}."
        elif channel_mlp_layers is not None:
            channel_mlp_layers = list(channel_mlp_layers)
            if channel_mlp_layers[0] != kernel_in_dim:
                channel_mlp_layers = [kernel_in_dim] + channel_mlp_layers
            if channel_mlp_layers[-1] != self.out_channels:
                channel_mlp_layers.append(self.out_channels)
            channel_mlp = LinearChannelMLP(layers=channel_mlp_layers, non_linearity=channel_mlp_non_linearity)
        self.integral_transform = IntegralTransform(channel_mlp=channel_mlp, transform_type=transform_type,
                                                    use_torch_scatter=use_torch_scatter_reduce,
                                                    weighting_fn=weighting_fn, reduction=reduction,
                                                    kernel_route="auto")

    def forward(self, y, x, f_y=None):
        neighbors = self.neighbor_search(data=y, queries=x, radius=self.radius)
        if self.pos_embedding is not None:
            y_embed, x_embed = self.pos_embedding(y), self.pos_embedding(x)
        else:
            y_embed, x_embed = y, x
        return self.integral_transform(y=y_embed, x=x_embed, neighbors=neighbors, f_y=f_y)
