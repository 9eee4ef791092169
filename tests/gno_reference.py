"""float64 restatement of the graph neural operator layer's formulas (neuralop/layers/neighbor_search.py,
segment_csr.py, integral_transform.py) for the tests: brute-force radius search, CSR reduce, the four transforms through
a dense MLP, and the case tables the recorder and the tests share.  numpy / torch on the host, no engine."""
import os

import numpy as np
import torch
import torch.nn.functional as F

# tile constants of sc_kernels_gno.h the search shapes are cut from
GNO_TILE, GNO_QPB = 1024, 32
BAND = 1e-5                       # relative width of the |dist - r| band inside which fp32 and float64 may disagree


def radius_search(data, queries, radius, return_norm=False):
    """The reference's native_neighbor_search in float64: dist <= radius, zero distances kept (weight eps^2 = 1e-14)"""
    data, queries = np.asarray(data, np.float64), np.asarray(queries, np.float64)
    dist = np.sqrt(((queries[:, None, :] - data[None, :, :]) ** 2).sum(-1)) if len(data) and len(queries) \
        else np.zeros((len(queries), len(data)))
    hit = dist <= radius
    rows, cols = np.nonzero(hit)
    out = {"neighbors_index": cols.astype(np.int64),
           "neighbors_row_splits": np.concatenate([[0], np.cumsum(hit.sum(1))]).astype(np.int64)}
    if return_norm:
        d = dist[rows, cols]
        out["weights"] = np.where(d == 0.0, 1e-7, d) ** 2
    return out


def band_queries(data, queries, radius, rel=BAND):
    """queries with some data point at |dist - r| <= rel r: the fp32 test d2 <= r2 may decide those either way"""
    data, queries = np.asarray(data, np.float64), np.asarray(queries, np.float64)
    dist = np.sqrt(((queries[:, None, :] - data[None, :, :]) ** 2).sum(-1))
    return (np.abs(dist - radius) <= rel * radius).any(1)


def random_csr(rng, rows, cols, lengths):
    """CSR with the given segment lengths; indices drawn with repetition, rows unsorted"""
    splits = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    assert len(lengths) == rows
    return splits, rng.integers(0, cols, size=int(splits[-1])).astype(np.int64)


def csr_reduce(K, splits, F_=None, index=None, w=None, mean=False):
    """out[(b,) i] = s_i sum_e K[(b,) e] F[(b,) index[e]] w[e] in float64"""
    K = np.asarray(K, np.float64)
    v = K
    if F_ is not None:
        v = v * np.asarray(F_, np.float64)[..., index, :]
    if w is not None:
        v = v * np.asarray(w, np.float64)[:, None]
    rows = len(splits) - 1
    out = np.zeros(v.shape[:-2] + (rows, v.shape[-1]))
    for i in range(rows):
        lo, hi = splits[i], splits[i + 1]
        if hi > lo:
            s = v[..., lo:hi, :].sum(-2)
            out[..., i, :] = s / (hi - lo) if mean else s
    return out


def transpose_csr(splits, index, cols):
    """col_splits, perm (edge ids by column, ascending), row_of_edge"""
    row = np.repeat(np.arange(len(splits) - 1), np.diff(splits))
    perm = np.argsort(index, kind="stable")
    col_splits = np.concatenate([[0], np.cumsum(np.bincount(index, minlength=cols))]).astype(np.int64)
    return col_splits, perm, row


def lattice_points(rng, n, m, d, L):
    """data (n, d) and queries (m, d) with coordinates k / L, k an integer in [0, L): for L a power of two differences,
    squares and their sums are exact in fp32 and in float64, so is r^2 for r = j / L -- pairs at distance exactly r and
    coincident pairs occur, and fp32 decides every one of them as float64 does (no band)."""
    data = rng.integers(0, L, size=(n, d)) / L
    queries = rng.integers(0, L, size=(m, d)) / L
    return data.astype(np.float32), queries.astype(np.float32)


def squared_distances(data, queries):
    """float64 [m, n]; exact for lattice_points"""
    data, queries = np.asarray(data, np.float64), np.asarray(queries, np.float64)
    return ((queries[:, None, :] - data[None, :, :]) ** 2).sum(-1)


def csr_reduce_torch(K, splits, F_=None, index=None, w=None, mean=False):
    """csr_reduce as a torch formula autograd can differentiate (float64 in, float64 out): K (E, c) or (b, E, c), F_
    None, (n, c) or (b, n, c); an empty row gives 0 under mean.  splits / index: int64 tensors."""
    v = K
    if F_ is not None:
        v = v * F_[..., index, :]
    if w is not None:
        v = v * w.unsqueeze(-1)
    rows = splits.numel() - 1
    deg = splits[1:] - splits[:-1]
    rep = torch.repeat_interleave(torch.arange(rows), deg)
    out = torch.zeros(v.shape[:-2] + (rows, v.shape[-1]), dtype=v.dtype).index_add(-2, rep, v)
    if mean:
        out = out / deg.to(v.dtype).clamp(min=1).unsqueeze(-1)
    return out


def sinusoidal_embedding(x, num_frequencies, max_positions=10000):
    """neuralop/layers/embeddings.py SinusoidalEmbedding, type "transformer", in the dtype of x (n, d) -> (n, 2 d nf):
    [sin(x_i w_k), cos(x_i w_k)] with w_k = max_positions^(-2 k / nf), k fastest but for the sin / cos pair"""
    k = torch.arange(num_frequencies, dtype=x.dtype)
    freqs = (1.0 / max_positions) ** (k / num_frequencies * 2)
    ang = x.unsqueeze(-1) * freqs
    return torch.stack((ang.sin(), ang.cos()), dim=-1).reshape(x.shape[0], -1)


def mlp_forward(weights, biases, x, act=F.gelu):
    for i, (W, b) in enumerate(zip(weights, biases)):
        x = F.linear(x, W, b)
        if i < len(weights) - 1:
            x = act(x)
    return x


def integral_transform(y, x, nbrs, weights, biases, f_y=None, transform_type="linear", reduction="sum",
                       weighting_fn=None, act=F.gelu):
    """The reference's IntegralTransform.forward as a dense float64 torch formula (autograd-capable): tensors in,
    tensor out; nbrs holds torch int64 arrays (and optionally weights)."""
    idx, splits = nbrs["neighbors_index"], nbrs["neighbors_row_splits"]
    rep = torch.repeat_interleave(torch.arange(x.shape[0]), splits[1:] - splits[:-1])
    agg = torch.cat([y[idx], x[rep]], dim=-1)
    nonlinear = f_y is not None and transform_type in ("nonlinear", "nonlinear_kernelonly")
    if nonlinear:
        if f_y.ndim == 3:
            agg = agg.unsqueeze(0).expand(f_y.shape[0], -1, -1)
        agg = torch.cat([agg, f_y[..., idx, :]], dim=-1)
    k = mlp_forward(weights, biases, agg, act)
    if f_y is not None and transform_type != "nonlinear_kernelonly":
        k = k * f_y[..., idx, :]
    w = nbrs.get("weights")
    if w is not None:
        k = k * (weighting_fn(w) if weighting_fn is not None else w).unsqueeze(-1)
        reduction = "sum"
    out = torch.zeros(k.shape[:-2] + (x.shape[0], k.shape[-1]), dtype=k.dtype)
    out = out.index_add(-2, rep, k)
    if reduction == "mean":
        deg = (splits[1:] - splits[:-1]).to(k.dtype).clamp(min=1).unsqueeze(-1)
        out = out / deg
    return out


def half_cos(x, radius=1.0, scale=1.0):
    return scale * (0.5 * torch.cos(torch.pi * (x / radius)) + 0.5)


# ---- recorded cases (tests/record_gno.py writes tests/golden/gno_<name>.npz) -----------------------------------------
# name: dict(d, n, m, radius, transform_type, reduction, weighting, pos (None / transformer / nerf), in_ch, out_ch,
#            layers, batch (0 = unbatched f_y, None = no f_y), special)
def _case(d, n, m, radius, tt, red="sum", weighting=None, pos=None, in_ch=3, out_ch=3, layers=(16, 8), batch=2,
          special=None, relu=False):
    return dict(d=d, n=n, m=m, radius=radius, transform_type=tt, reduction=red, weighting=weighting, pos=pos,
                in_ch=in_ch, out_ch=out_ch, layers=list(layers), batch=batch, special=special, relu=relu)


CASES = {
    "2d_linear_sum": _case(2, 48, 36, 0.25, "linear"),
    "2d_linear_mean_unbatched": _case(2, 48, 36, 0.25, "linear", red="mean", batch=0),
    "3d_linear_mean_transformer": _case(3, 60, 40, 0.4, "linear", red="mean", pos="transformer"),
    "3d_linear_halfcos": _case(3, 60, 40, 0.4, "linear", weighting="half_cos"),
    "3d_kernelonly_sum": _case(3, 50, 30, 0.35, "linear_kernelonly", batch=None),
    "2d_kernelonly_mean_nerf": _case(2, 40, 50, 0.2, "linear_kernelonly", red="mean", pos="nerf", batch=None),
    "3d_nonlinear_sum": _case(3, 50, 30, 0.35, "nonlinear"),
    "3d_nonlinear_mean_unbatched": _case(3, 50, 30, 0.35, "nonlinear", red="mean", batch=0),
    "2d_nonlinear_halfcos_transformer": _case(2, 48, 36, 0.25, "nonlinear", weighting="half_cos", pos="transformer"),
    "3d_nonlinear_kernelonly_sum": _case(3, 50, 30, 0.35, "nonlinear_kernelonly", out_ch=5),
    "2d_nonlinear_kernelonly_mean_halfcos": _case(2, 48, 36, 0.25, "nonlinear_kernelonly", red="mean",
                                                  weighting="half_cos", out_ch=4),
    "2d_linear_relu_custom_mlp": _case(2, 48, 36, 0.25, "linear", relu=True),
    "3d_linear_empty_neighbourhood": _case(3, 40, 30, 0.3, "linear", red="mean", special="empty"),
    "2d_linear_coincident": _case(2, 40, 30, 0.25, "linear", weighting="half_cos", special="coincident"),
    "3d_linear_x_is_y": _case(3, 45, 45, 0.35, "linear", special="x_is_y"),
}


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


# ---- the verbatim reference, where it exists --------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def reference_available():
    from oracle import ref_verbatim
    return os.path.isfile(os.path.join(ref_verbatim.REFERENCE_ROOT, "neuralop", "layers", "gno_block.py"))


def load_reference_gno():
    """(gno_block module, gno_weighting_functions module), verbatim, loaded from where they lie; their relative imports
    (neighbor_search, segment_csr, integral_transform, channel_mlp, embeddings) resolve through the same package path"""
    import importlib
    import sys
    import types
    from oracle import ref_verbatim
    root = os.path.join(ref_verbatim.REFERENCE_ROOT, "neuralop")
    for name, path in (("neuralop", root), ("neuralop.layers", os.path.join(root, "layers"))):
        if name not in sys.modules:
            pkg = types.ModuleType(name)
            pkg.__path__ = [path]
            sys.modules[name] = pkg
    return (importlib.import_module("neuralop.layers.gno_block"),
            importlib.import_module("neuralop.layers.gno_weighting_functions"))


def case_inputs(cfg, seed):
    """fp32-representable points, features and cotangent of a case"""
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(cfg["n"], cfg["d"], generator=g, dtype=torch.float32)
    x = torch.rand(cfg["m"], cfg["d"], generator=g, dtype=torch.float32)
    if cfg["special"] == "empty":
        x[2] = 5.0
    elif cfg["special"] == "coincident":
        x[1] = y[4]
        y[8] = y[7]
    elif cfg["special"] == "x_is_y":
        x = y
    f = None
    if cfg["batch"] is not None:
        f = torch.randn(*((cfg["batch"],) if cfg["batch"] else ()), cfg["n"], cfg["in_ch"], generator=g,
                        dtype=torch.float32)
    return y, x, f


def block_kwargs(cfg, weighting_fn, mlp_cls):
    kw = dict(in_channels=cfg["in_ch"], out_channels=cfg["out_ch"], coord_dim=cfg["d"], radius=cfg["radius"],
              transform_type=cfg["transform_type"], weighting_fn=weighting_fn, reduction=cfg["reduction"],
              pos_embedding_type=cfg["pos"], pos_embedding_channels=4, channel_mlp_layers=list(cfg["layers"]),
              use_torch_scatter_reduce=False, use_open3d_neighbor_search=False)
    if cfg["relu"]:
        k_in = (2 * cfg["d"] if cfg["pos"] is None else 16 * cfg["d"]) + \
            (cfg["in_ch"] if cfg["transform_type"].startswith("nonlinear") else 0)
        kw["channel_mlp"] = mlp_cls(layers=[k_in] + list(cfg["layers"]) + [cfg["out_ch"]], non_linearity=F.relu)
        # the reference's LinearChannelMLP carries neither attribute, its GNOBlock asserts on both
        kw["channel_mlp"].in_channels, kw["channel_mlp"].out_channels = k_in, cfg["out_ch"]
        kw["channel_mlp_layers"] = None
    return kw


def run_engine_case(cfg, rec, device):
    """neuraloperator_amd.GNOBlock on the recorded inputs and parameters: dict(out, nbrs, grads..., state)"""
    from functools import partial
    from neuraloperator_amd import GNOBlock
    from neuraloperator_amd.gno import LinearChannelMLP
    wfn = partial(half_cos, radius=cfg["radius"] ** 2, scale=1.0) if cfg["weighting"] == "half_cos" else None
    block = GNOBlock(**block_kwargs(cfg, wfn, LinearChannelMLP))
    state = {k[len("param:"):]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("param:")}
    block.load_state_dict(state, strict=True)
    block = block.to(device)
    assert block.integral_transform.lift_route() == (not cfg["relu"])
    y, x = torch.from_numpy(rec["y"]).to(device), torch.from_numpy(rec["x"]).to(device)
    if cfg["special"] == "x_is_y":
        x = y
    f = torch.from_numpy(rec["f_y"]).to(device).requires_grad_(True) if "f_y" in rec else None
    nbrs = block.neighbor_search(data=y, queries=x, radius=cfg["radius"])
    out = block(y, x, f)
    out.backward(torch.from_numpy(rec["g"]).float().to(device))
    res = {"out": out.detach().cpu().numpy(), "nbrs": {k: v.cpu().numpy() for k, v in nbrs.items()},
           "state": {k: tuple(v.shape) for k, v in block.state_dict().items()}}
    if f is not None:
        res["grad:f_y"] = f.grad.cpu().numpy()
    for k, p in block.named_parameters():
        res["grad:" + k] = p.grad.cpu().numpy()
    return res


def check_case_against_record(res, rec):
    """the bars of the issue: neighbour dicts exactly; 1e-5 outputs and input gradients; 2e-5 parameter gradients"""
    np.testing.assert_array_equal(res["nbrs"]["neighbors_index"], rec["nbr:neighbors_index"])
    np.testing.assert_array_equal(res["nbrs"]["neighbors_row_splits"], rec["nbr:neighbors_row_splits"])
    assert res["nbrs"]["neighbors_index"].dtype == np.int64 and res["nbrs"]["neighbors_row_splits"].dtype == np.int64
    if "nbr:weights" in rec:
        np.testing.assert_allclose(res["nbrs"]["weights"], rec["nbr:weights"], rtol=1e-6, atol=0)
    else:
        assert "weights" not in res["nbrs"]
    assert res["out"].shape == rec["ref:out"].shape
    errs = {"out": rel_l2(res["out"], rec["ref:out"])}
    assert errs["out"] <= 1e-5, errs
    for k in rec:
        if k.startswith("ref:grad:"):
            name = k[len("ref:"):]
            errs[name] = rel_l2(res[name], rec[k])
            assert errs[name] <= (1e-5 if name == "grad:f_y" else 2e-5), errs
    assert sorted(res["state"]) == sorted(str(s) for s in rec["state_keys"])
    for k, shp in zip(rec["state_keys"], rec["state_shapes"]):
        assert res["state"][str(k)] == tuple(int(v) for v in str(shp).split(",") if v), k
    return errs
