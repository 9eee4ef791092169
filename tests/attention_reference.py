"""Helper of the attention kernel integral tests: a float64 restatement of the forward pass written from the formula

    kn = LN_D(k), vn = LN_D(v);  dots[b, h] = sum_n (R kn)^T vn;  u = ((R q) dots) w

(gradients by autograd of that restatement in float64), the case tables of the fixtures (tests/record_attention.py,
tests/golden/attn_*.npz) and of the free-standing descriptors, rel_l2, and a mirror of the host plan's chunking so that
tests can name tile and chunk edges.  The rotary angle is DEFINED by two fp32 products, (coordinate fl32(scale /
min_freq)) inv_freq[i]; the helper forms it so and takes sine and cosine of it in float64."""
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

CHUNK = 256          # ATT_CHUNK (sc_kernels_attn.h): points of one partial of a D x D sum
TILE = 32            # points a workgroup stages at a time on the vector route (and in every D x D sum)
VECTOR, MFMA = 1, 2  # SC_ATTN_PATH_VECTOR, SC_ATTN_PATH_MFMA
KSTEP = 2            # points one matrix instruction consumes
BAR = 1e-5


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def route_of(d):
    """the route of a legal descriptor by its head_dim, as att_plan picks it"""
    return MFMA if d in (32, 64, 128) else VECTOR


def mfma_tile(d):
    """points of a tile of the per-point kernels on the matrix-core route"""
    return 64 if d == 128 else 128


def chunks(n):
    """number of partials of a sum over n points, as att_plan (sc_host_attn.h) cuts them"""
    return (n + CHUNK - 1) // CHUNK


def golden_path(name):
    return os.path.join(GOLDEN, "attn_" + name + ".npz")


def load_record(name):
    """the record of a case; a compact case keeps its gradients in a second file"""
    rec = dict(np.load(golden_path(name)))
    if os.path.isfile(golden_path(name + ".grads")):
        rec.update(np.load(golden_path(name + ".grads")))
    return rec


# ----------------------------------------------------------------------------------------------------------------------
# float64 restatement
# ----------------------------------------------------------------------------------------------------------------------
def layer_norm64(x):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5)


def rotate64(t, pos, inv_freq, rot_scale, rotary):
    """t [B, N, H, D] float64, pos [B, N, rotary] fp32, inv_freq fp32 [D / (2 rotary)]"""
    if not rotary:
        return t
    Q = t.shape[-1] // (2 * rotary)
    assert inv_freq.numel() == Q and pos.dtype == torch.float32 and inv_freq.dtype == torch.float32
    out = []
    for ax in range(rotary):
        ang = ((pos[..., ax] * torch.tensor(rot_scale, dtype=torch.float32))[..., None] * inv_freq).double()
        c, s = ang.cos()[:, :, None, :], ang.sin()[:, :, None, :]
        x1, x2 = t[..., 2 * Q * ax:2 * Q * ax + Q], t[..., 2 * Q * ax + Q:2 * Q * (ax + 1)]
        out += [x1 * c - x2 * s, x2 * c + x1 * s]
    return torch.cat(out, -1)


def core64(q, k, v, pos_src, pos_qry, inv_freq, rot_scale, weights, heads, rotary):
    """(u [B, n_qry, H D], dots [B, H, D, D]) in float64; weights [B, n_qry] by query row, or None = 1 / n_src"""
    B, ns, hd = k.shape
    D = hd // heads
    q4, k4, v4 = (t.double().reshape(B, -1, heads, D) for t in (q, k, v))
    kr = rotate64(layer_norm64(k4), pos_src, inv_freq, rot_scale, rotary)
    vn = layer_norm64(v4)
    qr = rotate64(q4, pos_qry, inv_freq, rot_scale, rotary)
    dots = torch.einsum("bnhi,bnhj->bhij", kr, vn)
    u = torch.einsum("bnhi,bhij->bnhj", qr, dots)
    w = 1.0 / ns if weights is None else weights.double().reshape(B, -1, 1, 1)
    return (u * w).reshape(B, -1, hd), dots


def core_with_grads64(q, k, v, pos_src, pos_qry, inv_freq, rot_scale, weights, heads, rotary, g):
    """(u, dots, g_q, g_k, g_v) in float64"""
    qq, kk, vv = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    u, dots = core64(qq, kk, vv, pos_src, pos_qry, inv_freq, rot_scale, weights, heads, rotary)
    u.backward(g.double())
    return u.detach(), dots.detach(), qq.grad, kk.grad, vv.grad


def rotary_of(m, emb, pos_dim):
    """(rotary, inv_freq, rot_scale) as the layer hands them to the engine"""
    if emb is None:
        return 0, None, 1.0
    return pos_dim, emb.inv_freq.detach().float().cpu(), float(emb.scale / emb.min_freq)


def layer_with_grads64(m, emb, u_src, pos_src, u_qry, pos_qry, weights, g):
    """the whole layer in float64 on the host from the module's fp32 parameters: (out, {name: gradient}) with the
    gradients of u_src, u_qry (where given) and every parameter"""
    params = {n: p.detach().cpu().double().clone().requires_grad_(True) for n, p in m.named_parameters()}
    xs = u_src.detach().cpu().double().clone().requires_grad_(True)
    xq = None if u_qry is None else u_qry.detach().cpu().double().clone().requires_grad_(True)
    qry = xs if xq is None else xq
    ps = pos_src.detach().cpu()
    pq = ps if pos_qry is None else pos_qry.detach().cpu()
    q = F.linear(qry, params["to_q.weight"]) if m.project_query else qry
    k, v = F.linear(xs, params["to_k.weight"]), F.linear(xs, params["to_v.weight"])
    rotary, inv_freq, rot_scale = rotary_of(m, emb, ps.shape[-1])
    w = None if weights is None else weights.detach().cpu().reshape(xs.shape[0], -1)
    u, _ = core64(q, k, v, ps, pq, inv_freq, rot_scale, w, m.n_heads, rotary)
    if "to_out.weight" in params:
        u = F.linear(u, params["to_out.weight"], params["to_out.bias"])
    u.backward(g.detach().cpu().double())
    grads = {n: p.grad for n, p in params.items()}
    grads["u_src"] = xs.grad
    if xq is not None:
        grads["u_qry"] = xq.grad
    return u.detach(), grads


# ----------------------------------------------------------------------------------------------------------------------
# fixtures: layers against the verbatim reference (tests/record_attention.py)
# ----------------------------------------------------------------------------------------------------------------------
def case(in_channels, out_channels, heads, d, n, batch, pos_dim=2, rotary=True, cross=False, weights=False,
         project_query=True, unit_pos=False, kernel=False, compact=False):
    return dict(in_channels=in_channels, out_channels=out_channels, heads=heads, d=d, n=n, batch=batch, pos_dim=pos_dim,
                rotary=rotary, cross=cross, weights=weights, project_query=project_query, unit_pos=unit_pos,
                kernel=kernel, compact=compact)


CASES = {
    # the reference's own test shape: D == in_channels (diagonal initialisation), to_out a Linear, randn positions
    "self_rot2_reference_shape": case(32, 32, 4, 32, 64, 4, compact=True),
    "self_rot2_unit_positions_d12": case(16, 24, 2, 12, 80, 2, unit_pos=True),            # to_out Identity, D != C
    "self_no_rotary_h3_d4": case(20, 12, 3, 4, 50, 2, rotary=False),
    "self_rot1_batch1_d12": case(12, 8, 1, 12, 40, 1, pos_dim=1, kernel=True),             # diagonal, Linear out
    "cross_rot2_d32": case(16, 64, 2, 32, 48, 2, cross=True),
    "cross_no_rotary_d12": case(10, 7, 2, 12, 33, 3, cross=True, rotary=False),
    "weights_rot2_h1_d64": case(8, 64, 1, 64, 96, 2, weights=True, unit_pos=True),
    "cross_weights_no_query_projection_d4": case(10, 8, 2, 4, 31, 2, cross=True, weights=True, project_query=False),
    "self_rot2_h3_d4_diagonal": case(4, 12, 3, 4, 30, 2, kernel=True),
    "self_rot2_linear_out_d64": case(24, 5, 2, 64, 65, 1),
    "weights_no_rotary_d32": case(32, 32, 1, 32, 72, 2, rotary=False, weights=True),
}
SEEDS = {name: 8100 + i for i, name in enumerate(sorted(CASES))}


def case_inputs(cfg, seed):
    """fp32 inputs of a case: dict with u_src, pos_src, g and, as the case has them, u_qry, pos_qry, weights"""
    gen = torch.Generator().manual_seed(seed + 1)
    B, n = cfg["batch"], cfg["n"]

    def positions():
        if cfg["unit_pos"]:
            return torch.rand(B, n, cfg["pos_dim"], generator=gen)
        return torch.randn(B, n, cfg["pos_dim"], generator=gen)

    out = {"u_src": torch.randn(B, n, cfg["in_channels"], generator=gen), "pos_src": positions()}
    if cfg["cross"]:
        cq = cfg["in_channels"] if cfg["project_query"] else cfg["heads"] * cfg["d"]
        out["u_qry"] = torch.randn(B, n, cq, generator=gen)
        out["pos_qry"] = positions()
    if cfg["weights"]:
        out["weights"] = torch.rand(B, n, generator=gen) * (2.0 / n)
    out["g"] = torch.randn(B, n, cfg["out_channels"], generator=gen)
    return out


def build_layer(cls, emb_cls, cfg, seed):
    """the layer as initialised under the case's seed, and its rotary module (or None)"""
    torch.manual_seed(seed)
    m = cls(cfg["in_channels"], cfg["out_channels"], cfg["heads"], cfg["d"], project_query=cfg["project_query"])
    emb = emb_cls(cfg["d"] // cfg["pos_dim"]) if cfg["rotary"] else None
    return m, emb


def call_layer(m, emb, t, **kw):
    return m(t["u_src"], t["pos_src"], positional_embedding_module=emb, u_qry=t.get("u_qry"), pos_qry=t.get("pos_qry"),
             weights=t.get("weights"), **kw)


def grads_of(m, t):
    """{name: gradient} after a backward pass: inputs that require grad and every parameter"""
    out = {"u_src": t["u_src"].grad}
    if t.get("u_qry") is not None:
        out["u_qry"] = t["u_qry"].grad
    out.update({n: p.grad for n, p in m.named_parameters()})
    return out


def tolerance(rec, key):
    """the bar of a tensor against the record.  It was to be max(1e-5, 2 x the recorded error of the verbatim fp32 module
    against its float64 run); the recorder shows every such error below 5e-6 (the worst over all cases and tensors is
    4.7e-7, randn positions with angles of 200 radians included), so the second term is dropped: 1e-5 flat.  The
    recorded errors stay in the files, and every one is checked to be below 5e-6 here."""
    assert float(rec["err:" + key]) < 5e-6, (key, float(rec["err:" + key]))
    return BAR


# ----------------------------------------------------------------------------------------------------------------------
# free-standing descriptors through the C-ABI
# ----------------------------------------------------------------------------------------------------------------------
def desc_case(batch=1, n_src=40, n_qry=None, heads=1, d=4, rotary=2, weights=False, zero_point=None):
    return dict(batch=batch, n_src=n_src, n_qry=n_src if n_qry is None else n_qry, heads=heads, d=d, rotary=rotary,
                weights=weights, zero_point=zero_point)


DESC_CASES = {
    "n_one_below_a_chunk_d4_rot2": desc_case(n_src=CHUNK - 1),
    "n_a_chunk_d2_rot1": desc_case(n_src=CHUNK, d=2, rotary=1),
    "n_one_above_a_chunk_d12_h2_rot2_weights": desc_case(n_src=CHUNK + 1, heads=2, d=12, weights=True),
    "n_one_above_two_chunks_d4_no_rotary": desc_case(n_src=2 * CHUNK + 1, rotary=0),
    "n_one_point_d32_rot2": desc_case(n_src=1, d=32),
    "n_one_above_a_tile_d32_rot1": desc_case(n_src=TILE + 1, d=32, rotary=1),
    "batch3_h3_d12_rot1": desc_case(batch=3, heads=3, d=12, rotary=1),                     # H D = 36
    "cross_70_to_45_d32_h2_rot2_weights": desc_case(n_src=70, n_qry=45, heads=2, d=32, weights=True),
    "cross_9_to_300_d4_no_rotary": desc_case(n_src=9, n_qry=300, rotary=0),
    "zero_point_d4_rot2": desc_case(n_src=50, heads=2, zero_point=7),
    "d36_second_lane_layout_no_rotary": desc_case(n_src=33, d=36, rotary=0, weights=True),
    "d68_third_lane_layout_rot2": desc_case(n_src=35, d=68),
    # matrix-core route: a point count that is no multiple of the K-step, one past a tile of the per-point kernels
    "mfma_d32_odd_points_rot2": desc_case(n_src=2 * TILE + KSTEP + 1, d=32, heads=2),
    "mfma_d32_one_past_a_tile_cross_weights": desc_case(n_src=129, n_qry=77, d=32, rotary=1, weights=True),
    "mfma_d64_odd_points_no_rotary": desc_case(n_src=37, d=64, rotary=0, batch=2),
    "mfma_d128_one_past_a_tile_rot2": desc_case(n_src=65, d=128),
}


def desc_inputs(cfg, seed):
    """(q, k, v, pos_src, pos_qry, inv_freq, rot_scale, weights, g) fp32 on the host; positions in [0, 1) at the module's
    default scale / min_freq = 64, so angles reach 64 radians"""
    gen = torch.Generator().manual_seed(seed)
    B, ns, nq, hd, r = cfg["batch"], cfg["n_src"], cfg["n_qry"], cfg["heads"] * cfg["d"], cfg["rotary"]
    q, k, v = (torch.randn(B, n, hd, generator=gen) for n in (nq, ns, ns))
    k = k * 0.7 + 0.3                                                     # a mean the norm has to remove
    if cfg["zero_point"] is not None:
        k[:, cfg["zero_point"]] = 0.0
        v[:, cfg["zero_point"]] = 0.0
    pos_src = pos_qry = inv_freq = None
    if r:
        pos_src, pos_qry = torch.rand(B, ns, r, generator=gen), torch.rand(B, nq, r, generator=gen)
        dim = cfg["d"] // r
        inv_freq = 1.0 / (10000 ** (torch.arange(0, dim, 2).float() / dim))
    weights = torch.rand(B, nq, generator=gen) * (2.0 / ns) if cfg["weights"] else None
    g = torch.randn(B, nq, hd, generator=gen)
    return q, k, v, pos_src, pos_qry, inv_freq, 64.0, weights, g


def desc_of(cfg, **change):
    from neuraloperator_amd import _lib
    kw = dict(batch=cfg["batch"], n_src=cfg["n_src"], n_qry=cfg["n_qry"], heads=cfg["heads"], head_dim=cfg["d"],
              rotary=cfg["rotary"], has_weights=int(cfg["weights"]))
    kw.update(change)
    return _lib.ScEngineLib.attn_desc(**kw)


def run_descriptor(lib, cfg, q, k, v, pos_src, pos_qry, inv_freq, rot_scale, weights, g, want=(True, True, True),
                   device="cpu"):
    """sc_attn_forward + sc_attn_backward on tensors moved to `device`: (u, dots, gq, gk, gv) back on the host, None for
    a gradient that was not asked for"""
    dev = torch.device(device)
    mv = lambda t: None if t is None else t.to(dev).contiguous()                        # noqa: E731
    q, k, v, pos_src, pos_qry, inv_freq, weights, g = (mv(t) for t in (q, k, v, pos_src, pos_qry, inv_freq, weights, g))
    d = desc_of(cfg)
    assert lib.attn_path(d) == route_of(cfg["d"])
    nbytes = lib.attn_workspace_bytes(d)
    assert nbytes == 4 * cfg["batch"] * cfg["heads"] * cfg["d"] ** 2 * (max(chunks(cfg["n_src"]), chunks(cfg["n_qry"])) + 3)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream().cuda_stream if dev.type == "cuda" else 0
    p = lambda t: 0 if t is None else t.data_ptr()                                      # noqa: E731
    u = torch.full_like(q, float("nan"))
    dots = torch.full((cfg["batch"], cfg["heads"], cfg["d"], cfg["d"]), float("nan"), device=dev)
    lib.attn_forward(d, p(q), p(k), p(v), p(pos_src), p(pos_qry), p(inv_freq), rot_scale, p(weights), p(u), p(dots),
                     p(ws), nbytes, st)
    grads = [torch.full_like(t, float("nan")) if w else None for t, w in zip((q, k, v), want)]
    lib.attn_backward(d, p(q), p(k), p(v), p(pos_src), p(pos_qry), p(inv_freq), rot_scale, p(weights), p(dots), p(g),
                      p(grads[0]), p(grads[1]), p(grads[2]), p(ws), nbytes, st)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in [u, dots] + grads)


def desc_errors(got, cfg, args):
    """rel-L2 of (u, dots, gq, gk, gv) against the float64 helper, by name"""
    q, k, v, pos_src, pos_qry, inv_freq, rot_scale, weights, g = args
    want = core_with_grads64(q, k, v, pos_src, pos_qry, inv_freq, rot_scale, weights, cfg["heads"], cfg["rotary"], g)
    return {n: rel_l2(a.numpy(), b.numpy()) for n, a, b in zip(("u", "dots", "gq", "gk", "gv"), got, want)
            if a is not None}
