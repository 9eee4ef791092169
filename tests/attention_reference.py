"""Helper of the attention kernel integral tests: a float64 restatement of the forward pass written from the formula

    kn = LN_D(k), vn = LN_D(v);  dots[b, h] = sum_n (R kn)^T vn;  u = ((R q) dots) w

(gradients by autograd of that restatement in float64), the case tables of the fixtures (tests/record_attention.py,
tests/golden/attn_*.npz) and of the free-standing descriptors, rel_l2, and a mirror of the host plan's chunking so that
tests can name tile and chunk edges.  The rotary angle is DEFINED by two fp32 products, (coordinate fl32(scale /
min_freq)) inv_freq[i]; the helper forms it so and takes sine and cosine of it in float64.

For the kernel-edge tests (tests/test_gpu_attention_kernels.py, tests/test_emu_attention.py) it also holds: the launch
constants read off sc_kernels_attn.h / sc_host_attn.h, the table ATTN_KERNEL_CASES, run_descriptor(guard=True) on
buffers between NaN guard bands with the workspace's intermediates read back, the per-element bounds (N, A) of DESIGN
3.26 (reference_with_bounds, check_levels) and the formula in plain fp32 (manual_core)."""
import os
import re

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
U = 2.0 ** -24       # unit roundoff of fp32


def _kernel_constants():
    """ATT_CHUNK, the 32-point tile, ATT_MTP(DP) and the K-step as sc_kernels_attn.h and sc_host_attn.h state them"""
    csrc = os.path.join(os.path.dirname(HERE), "neuraloperator_amd", "csrc")
    with open(os.path.join(csrc, "sc_kernels_attn.h")) as f:
        kern = f.read()
    with open(os.path.join(csrc, "sc_host_attn.h")) as f:
        host = f.read()
    chunk = int(re.search(r"^#define ATT_CHUNK (\d+)", kern, re.M).group(1))
    tiles = {int(t) for t in re.findall(r"constexpr int TP = (?:MF \? ATT_MTP\(DP\) : )?(\d+)\b", kern)}
    tiles |= {int(t) for t in re.findall(r"\? ATT_MTP\(p\.DP\) : (\d+);", host)}
    assert len(tiles) == 1, tiles
    m = re.search(r"^#define ATT_MTP\(DP\) \(\(DP\) == 128 \? (\d+) : (\d+)\)", kern, re.M)
    mtp = {32: int(m.group(2)), 64: int(m.group(2)), 128: int(m.group(1))}
    ksteps = {int(t) for t in re.findall(r"for \(int p = p0; p < p1; p \+= (\d+)\)", kern)}
    ksteps |= {int(t) for t in re.findall(r"v_mfma_f32_32x32x(\d+)_f32", kern)}
    assert len(ksteps) == 1, ksteps
    assert "parts | dots^T | g_dots | g_dots^T" in host and "p.bh * c * p.dd + 3 * p.bh * p.dd" in host
    assert "att_fwd_floats(const AttPlan& p) { return (size_t)(p.bh * p.chunks_src * p.dd); }" in host
    return chunk, tiles.pop(), mtp, ksteps.pop()


def gamma(n):
    return n * U / (1.0 - n * U)


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


def tile_of(d):
    """points of a tile of the per-point kernels (k_attn_apply, k_attn_kv_bwd[_mfma]) on the route of head_dim d"""
    return mfma_tile(d) if route_of(d) == MFMA else TILE


def dp_of(d):
    return 32 if d <= 32 else (64 if d <= 64 else 128)


_K = _kernel_constants()                                                  # a changed kernel constant fails here, at import
assert _K == (CHUNK, TILE, {d: mfma_tile(d) for d in (32, 64, 128)}, KSTEP), _K


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


def core_with_grads64(q, k, v, pos_src, pos_qry, inv_freq, rot_scale, weights, heads, rotary, g, with_g_dots=False):
    """(u, dots, g_q, g_k, g_v) in float64; with_g_dots: also g_dots [B, H, D, D] = sum_n (R q)^T (w g)"""
    qq, kk, vv = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    u, dots = core64(qq, kk, vv, pos_src, pos_qry, inv_freq, rot_scale, weights, heads, rotary)
    u.backward(g.double())
    out = (u.detach(), dots.detach(), qq.grad, kk.grad, vv.grad)
    if not with_g_dots:
        return out
    B, ns, hd = k.shape
    D = hd // heads
    qr = rotate64(q.double().reshape(B, -1, heads, D), pos_qry, inv_freq, rot_scale, rotary)
    w = 1.0 / ns if weights is None else weights.double().reshape(B, -1, 1, 1)
    return out + (torch.einsum("bnhi,bnhj->bhij", qr, g.double().reshape(B, -1, heads, D) * w),)


# ----------------------------------------------------------------------------------------------------------------------
# the same formula with fp32 roundings where the kernels round (the layer-norm backward in float64, as att_norm_bwd)
# ----------------------------------------------------------------------------------------------------------------------
def _norm_bwd_manual(gy, x64, dt):
    mu = x64.mean(-1, keepdim=True)
    r = torch.rsqrt(((x64 - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
    xn, g = (x64 - mu) * r, gy.double()
    return (r * (g - g.mean(-1, keepdim=True) - xn * (g * xn).mean(-1, keepdim=True))).to(dt)


def manual_core(q, k, v, pos_src, pos_qry, inv_freq, rot_scale, weights, heads, rotary, g, dt):
    """dict of u, dots, gq, gk, gv, dots_t, g_dots, g_dots_t by the kernels' own chain of passes, every tensor held in
    ``dt`` (torch.float32: the plain fp32 formula; torch.float64: a second statement of the helper, without autograd).
    Sine and cosine are float64 values rounded to ``dt``; the layer-norm backward is float64 rounded to ``dt``."""
    B, ns, hd = k.shape
    D = hd // heads
    q4, k4, v4, g4 = (t.to(dt).reshape(B, -1, heads, D) for t in (q, k, v, g))

    def ln(x):
        mu = x.mean(-1, keepdim=True)
        d = x - mu
        return d * torch.rsqrt((d * d).mean(-1, keepdim=True) + 1e-5)

    def rot(t, pos, sign):
        if not rotary:
            return t
        Q, out = D // (2 * rotary), []
        for ax in range(rotary):
            ang = ((pos[..., ax] * torch.tensor(rot_scale, dtype=torch.float32))[..., None] * inv_freq).double()
            c, s = ang.cos()[:, :, None, :].to(dt), (sign * ang.sin())[:, :, None, :].to(dt)
            x1, x2 = t[..., 2 * Q * ax:2 * Q * ax + Q], t[..., 2 * Q * ax + Q:2 * Q * (ax + 1)]
            out += [x1 * c - x2 * s, x2 * c + x1 * s]
        return torch.cat(out, -1)

    w = torch.tensor(1.0 / ns, dtype=dt) if weights is None else weights.to(dt).reshape(B, -1, 1, 1)
    kr, vn, qr = rot(ln(k4), pos_src, 1.0), ln(v4), rot(q4, pos_qry, 1.0)
    dots = torch.einsum("bnhi,bnhj->bhij", kr, vn)
    u = torch.einsum("bnhi,bhij->bnhj", qr, dots) * w
    wg = g4 * w
    gq = rot(torch.einsum("bnhj,bhij->bnhi", wg, dots), pos_qry, -1.0)
    gd = torch.einsum("bnhi,bnhj->bhij", qr, wg)
    gv = _norm_bwd_manual(torch.einsum("bnhi,bhij->bnhj", kr, gd), v.double().reshape(B, -1, heads, D), dt)
    gk = _norm_bwd_manual(rot(torch.einsum("bnhj,bhij->bnhi", vn, gd), pos_src, -1.0),
                          k.double().reshape(B, -1, heads, D), dt)
    flat = lambda t: t.reshape(B, -1, hd)                                               # noqa: E731
    return dict(u=flat(u), dots=dots, gq=flat(gq), gk=flat(gk), gv=flat(gv), dots_t=dots.transpose(-1, -2),
                g_dots=gd, g_dots_t=gd.transpose(-1, -2))


# ----------------------------------------------------------------------------------------------------------------------
# bounds: |computed - exact| <= gamma_N A per element.  A value that carries (N, A) with A >= |value| gives
#   a product   (N_x + N_y + 1, A_x A_y)          (the + 1 is the product's own rounding, or the fmaf's that takes it in)
#   a sum of m  (max N + m, sum A)                (at most one rounding per term, whatever the order)
# so A is the formula with every term replaced by its absolute value and N the roundings of the longest path.
# ----------------------------------------------------------------------------------------------------------------------
def _norm_bound(x, sub):
    """att_norm<TP, DP> with sub = 256 / TP sub-lanes on x [B, n, H, D] float64: (A_xn, N_xn)"""
    D = x.shape[-1]
    n_sum = -(-D // sub) + sub                                # a lane's ceil(D / S) terms, then the S sub-lane partials
    n_m, a_m = n_sum + 2, x.abs().mean(-1, keepdim=True)      # 1 / D and the product with it
    n_d, a_d = n_m + 1, x.abs() + a_m
    e_d = gamma(n_d) * a_d                                    # |d~ - d|, d = x - mean: the r u |x| term of a constant row
    d = (x - x.mean(-1, keepdim=True)).abs()
    s = (d * d).mean(-1, keepdim=True) + 1e-5
    r = torch.rsqrt(s)
    # s~ - s: d~ d~ - d d = 2 d e + e e per term (the product fused into its fmaf), then the sum's own roundings, 1 / D
    # and the fmaf with eps.  It is taken against |d|, not against A_d: a constant row has s = eps and A_d^2 / eps = 1e5
    n_s = 2 * n_d + n_sum + 2
    e_s = (2 * d * e_d + e_d * e_d).mean(-1, keepdim=True) + gamma(n_sum + 2) * (((d + e_d) ** 2).mean(-1, keepdim=True) + 1e-5)
    rho = e_s / s
    assert float(rho.max()) < 0.25
    # r = 1 / sqrt(s): (1 - rho)^(-1/2) - 1 <= 0.625 rho below rho = 1 / 4, and the square root's and the division's roundings
    e_r = rho + 3 * U
    e_xn = e_d * r * (1 + e_r) + d * r * e_r + U * (d + e_d) * r * (1 + e_r)
    n_xn = n_d + (n_s + 2) + 1
    return torch.maximum(d * r, e_xn / gamma(n_xn)), n_xn


def _rot_abs(a, pos, inv_freq, rot_scale, rotary):
    """A of a rotated row: |x1| |cos| + |x2| |sin| (the rotation's roundings are counted by the caller)"""
    if not rotary:
        return a
    Q, out = a.shape[-1] // (2 * rotary), []
    for ax in range(rotary):
        ang = ((pos[..., ax] * torch.tensor(rot_scale, dtype=torch.float32))[..., None] * inv_freq).double()
        c, s = ang.cos().abs()[:, :, None, :], ang.sin().abs()[:, :, None, :]
        x1, x2 = a[..., 2 * Q * ax:2 * Q * ax + Q], a[..., 2 * Q * ax + Q:2 * Q * (ax + 1)]
        out += [x1 * c + x2 * s, x2 * c + x1 * s]
    return torch.cat(out, -1)


def _norm_bwd_abs(x, a_g):
    mu = x.mean(-1, keepdim=True)
    r = torch.rsqrt(((x - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
    xn = ((x - mu) * r).abs()
    return r * (a_g + a_g.mean(-1, keepdim=True) + xn * (a_g * xn).mean(-1, keepdim=True))


ROT_N = 3      # a rotated element: two products and an add (the angle's two products are part of its definition)


def reference_with_bounds(cfg, args):
    """{name: (value, A, N)} in float64 for u, dots, gq, gk, gv, dots_t, g_dots, g_dots_t of a descriptor case.  The
    counts follow sc_kernels_attn.h stage by stage; with rotary they leave the error of sincosf out, so the
    element bound is asserted without rotary only."""
    q, k, v, pos_src, pos_qry, inv_freq, rot_scale, weights, g = args
    H, D, rotary = cfg["heads"], cfg["d"], cfg["rotary"]
    B, ns, nq = cfg["batch"], cfg["n_src"], cfg["n_qry"]
    u, dots, gq, gk, gv, gd = core_with_grads64(q, k, v, pos_src, pos_qry, inv_freq, rot_scale, weights, H, rotary, g,
                                                with_g_dots=True)
    q4, k4, v4, g4 = (t.double().reshape(B, -1, H, D) for t in (q, k, v, g))
    rn = ROT_N if rotary else 0
    comb = 3 if D == 32 else 0                                # k_attn_outer<32, true>: the four waves' sums, three adds
    rot = lambda a, pos: _rot_abs(a, pos, inv_freq, rot_scale, rotary)                  # noqa: E731
    # forward: k_attn_outer (TP = 32: 8 sub-lanes) + k_attn_reduce, k_attn_apply
    a_kn, n_kn = _norm_bound(k4, 256 // TILE)
    a_vn, n_vn = _norm_bound(v4, 256 // TILE)
    a_dots = torch.einsum("bnhi,bnhj->bhij", rot(a_kn, pos_src), a_vn)
    n_dots = (n_kn + rn) + n_vn + min(ns, CHUNK) + chunks(ns) - 1 + comb
    a_w = torch.full((1, 1, 1, 1), 1.0 / ns, dtype=torch.float64) if weights is None else \
        weights.double().abs().reshape(B, -1, 1, 1)
    n_w = 1 if weights is None else 0                         # 1 / n_src is rounded, a given weight is data
    a_qr = rot(q4.abs(), pos_qry)
    a_u, n_u = torch.einsum("bnhi,bhij->bnhj", a_qr, a_dots) * a_w, rn + n_dots + D + n_w + 1
    # backward: the query side
    a_wg, n_wg = g4.abs() * a_w, n_w + 1
    a_gq, n_gq = rot(torch.einsum("bnhj,bhij->bnhi", a_wg, a_dots), pos_qry), n_wg + n_dots + D + rn
    a_gd = torch.einsum("bnhi,bnhj->bhij", a_qr, a_wg)
    n_gd = rn + n_wg + min(nq, CHUNK) + chunks(nq) - 1 + comb
    # backward: the source side, k_attn_kv_bwd[_mfma] with 256 / tile sub-lanes in its norms
    sub = 256 // tile_of(D)
    (a_kn2, n_kn2), (a_vn2, n_vn2) = _norm_bound(k4, sub), _norm_bound(v4, sub)
    a_gv = _norm_bwd_abs(v4, torch.einsum("bnhi,bhij->bnhj", rot(a_kn2, pos_src), a_gd))
    a_gk = _norm_bwd_abs(k4, rot(torch.einsum("bnhj,bhij->bnhi", a_vn2, a_gd), pos_src))
    n_gv = (n_kn2 + rn) + n_gd + D + 2                        # att_norm_bwd: float64 (counted as one) and its rounding
    n_gk = n_vn2 + n_gd + D + rn + 2
    flat = lambda t: t.reshape(B, -1, H * D)                                            # noqa: E731
    return dict(u=(u, flat(a_u), n_u), dots=(dots, a_dots, n_dots), gq=(gq, flat(a_gq), n_gq),
                gk=(gk, flat(a_gk), n_gk), gv=(gv, flat(a_gv), n_gv),
                dots_t=(dots.transpose(-1, -2), a_dots.transpose(-1, -2), n_dots), g_dots=(gd, a_gd, n_gd),
                g_dots_t=(gd.transpose(-1, -2), a_gd.transpose(-1, -2), n_gd))


POINT_TENSORS = ("u", "gq", "gk", "gv")


def check_levels(label, cfg, got, ref, element=None):
    """level 1 on every tensor of ``got`` ({name: tensor}): rel-L2 <= BAR and, row by row (a point's head channels, a
    matrix row), ||err|| <= BAR ||A||; level 2 without rotary (or where ``element`` says so): |err| <= gamma_N A per
    element, exactly 0 where A is 0.  Returns {name: (rel-L2, worst row ratio, worst element ratio or None)}."""
    element = (cfg["rotary"] == 0) if element is None else element
    out, D = {}, cfg["d"]
    for name, t in got.items():
        if t is None:
            continue
        val, A, N = ref[name]
        t = t.double()
        assert t.shape == val.shape and bool(torch.isfinite(t).all()), (label, name)
        err = (t - val).abs()
        rows = lambda x: x.reshape(-1, D).norm(dim=-1)                                  # noqa: E731
        e_row, a_row = rows(err), rows(A)
        row = float((e_row / (BAR * a_row).clamp_min(1e-300)).max())
        rel = rel_l2(t.numpy(), val.numpy())
        el = float((err / (gamma(N) * A).clamp_min(1e-300)).max()) if element else None
        out[name] = (rel, row, el)
    print(label, " ".join(f"{n} {r:.1e}/{w:.3f}" + ("" if e is None else f"/{e:.3f}") for n, (r, w, e) in out.items()),
          "(rel-L2 / worst row / worst element, of their bounds)")
    for name, (rel, row, el) in out.items():
        assert rel <= BAR, (label, name, rel)
        assert row <= 1.0, (label, name, row)
        assert el is None or el <= 1.0, (label, name, el)
    return out


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
def desc_case(batch=1, n_src=40, n_qry=None, heads=1, d=4, rotary=2, weights=False, zero_point=None, mark_g=None,
              mark_q=None, const_row=None, emu=False):
    """weights: False, True, or "signed" (a zero and a negative entry); mark_g / mark_q: the one query row at which g / q
    is not zero; const_row: a source point whose k is constant over the channels of head 0; emu: the emulation tier runs
    the case too"""
    return dict(batch=batch, n_src=n_src, n_qry=n_src if n_qry is None else n_qry, heads=heads, d=d, rotary=rotary,
                weights=weights, zero_point=zero_point, mark_g=mark_g, mark_q=mark_q, const_row=const_row, emu=emu)


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
    # the marks of the kernel table, applied after every draw: the other cases' inputs are what they were
    if cfg["weights"] == "signed":
        weights[:, 0] = 0.0
        weights[:, 1 % nq] *= -1.0
    if cfg.get("const_row") is not None:
        k[:, cfg["const_row"], :cfg["d"]] = 0.8
    for t, row in ((g, cfg.get("mark_g")), (q, cfg.get("mark_q"))):
        if row is not None:
            keep = t[:, row].clone()
            t.zero_()
            t[:, row] = keep
    return q, k, v, pos_src, pos_qry, inv_freq, 64.0, weights, g


def desc_of(cfg, **change):
    from neuraloperator_amd import _lib
    kw = dict(batch=cfg["batch"], n_src=cfg["n_src"], n_qry=cfg["n_qry"], heads=cfg["heads"], head_dim=cfg["d"],
              rotary=cfg["rotary"], has_weights=int(bool(cfg["weights"])))
    kw.update(change)
    return _lib.ScEngineLib.attn_desc(**kw)


SENTINEL = 0x7FC0BEEF          # a NaN no kernel produces: the guards and the unwritten workspace are compared bit for bit


class Guarded:
    """a tensor of ``numel`` floats as a view into a buffer with ``pad`` sentinel floats in front and behind; the view
    itself starts as the sentinel too, so an element nobody wrote is a NaN"""

    def __init__(self, shape, pad, dev):
        self.numel, self.pad = int(np.prod(shape)), int(pad)
        self.buf = torch.full((self.numel + 2 * self.pad,), SENTINEL, dtype=torch.int32, device=dev)
        self.view = self.buf[self.pad:self.pad + self.numel].view(torch.float32).reshape(shape)

    def guards_intact(self):
        return bool((self.buf[:self.pad] == SENTINEL).all()) and bool((self.buf[self.pad + self.numel:] == SENTINEL).all())

    def untouched(self, lo=0, hi=None):
        """floats [lo, hi) of the view still hold the sentinel"""
        hi = self.numel if hi is None else hi
        return bool((self.buf[self.pad + lo:self.pad + hi] == SENTINEL).all())


def workspace_layout(cfg):
    """offsets in floats of parts | dots^T | g_dots | g_dots^T (the layout comment of sc_host_attn.h) and the total"""
    bh, dd = cfg["batch"] * cfg["heads"], cfg["d"] ** 2
    cmax = max(chunks(cfg["n_src"]), chunks(cfg["n_qry"]))
    dots_t = bh * cmax * dd
    return dict(dots_t=dots_t, g_dots=dots_t + bh * dd, g_dots_t=dots_t + 2 * bh * dd, total=dots_t + 3 * bh * dd, bhdd=bh * dd)


def _run_guarded(lib, cfg, dev, d, st, q, k, v, pos_src, pos_qry, inv_freq, rot_scale, weights, g, want):
    p = lambda t: 0 if t is None else t.data_ptr()                                      # noqa: E731
    B, H, D = cfg["batch"], cfg["heads"], cfg["d"]
    pad = tile_of(D) * H * D                                  # one full tile of rows
    lay = workspace_layout(cfg)
    assert lib.attn_workspace_bytes(d) == 4 * lay["total"]
    fwd_floats = lay["bhdd"] * chunks(cfg["n_src"])           # the forward call's own, smaller workspace
    u, dots = Guarded(q.shape, pad, dev), Guarded((B, H, D, D), pad, dev)
    ws_f, ws = Guarded((fwd_floats,), pad, dev), Guarded((lay["total"],), pad, dev)
    lib.attn_forward(d, p(q), p(k), p(v), p(pos_src), p(pos_qry), p(inv_freq), rot_scale, p(weights), p(u.view),
                     p(dots.view), p(ws_f.view), 4 * fwd_floats, st)
    grads = [Guarded(t.shape, pad, dev) for t in (q, k, v)]
    gp = [p(t.view) if w else 0 for t, w in zip(grads, want)]
    lib.attn_backward(d, p(q), p(k), p(v), p(pos_src), p(pos_qry), p(inv_freq), rot_scale, p(weights), p(dots.view),
                      p(g), gp[0], gp[1], gp[2], p(ws.view), 4 * lay["total"], st)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    for name, t in (("u", u), ("dots", dots), ("forward workspace", ws_f), ("workspace", ws), ("gq", grads[0]),
                    ("gk", grads[1]), ("gv", grads[2])):
        assert t.guards_intact(), "a store outside " + name
    for name, t, w in zip(("gq", "gk", "gv"), grads, want):
        assert w or t.untouched(), "a gradient that was not asked for was written: " + name
    # what the backward call has no reason to write: dots^T without gq; the partials past chunks_qry, g_dots and
    # g_dots^T without gk or gv
    kv = want[1] or want[2]
    assert ws.untouched(lay["bhdd"] * chunks(cfg["n_qry"]) if kv else 0, lay["dots_t"]), "partials region"
    assert want[0] or ws.untouched(lay["dots_t"], lay["g_dots"]), "dots^T was written without gq"
    assert kv or ws.untouched(lay["g_dots"], lay["total"]), "g_dots was written without gk or gv"
    region = lambda lo: ws.view[lo:lo + lay["bhdd"]].reshape(B, H, D, D).cpu()          # noqa: E731
    extra = dict(dots_t=region(lay["dots_t"]) if want[0] else None, g_dots=region(lay["g_dots"]) if kv else None,
                 g_dots_t=region(lay["g_dots_t"]) if kv else None)
    outs = [u.view.cpu(), dots.view.cpu()] + [t.view.cpu() if w else None for t, w in zip(grads, want)]
    return tuple(outs) + (extra,)


def run_descriptor(lib, cfg, q, k, v, pos_src, pos_qry, inv_freq, rot_scale, weights, g, want=(True, True, True),
                   device="cpu", guard=False):
    """sc_attn_forward + sc_attn_backward on tensors moved to `device`: (u, dots, gq, gk, gv) back on the host, None for
    a gradient that was not asked for.  guard=True: every output and both workspaces are views into larger buffers with
    a full tile of rows of a NaN sentinel on both sides, compared bit for bit after the calls; a gradient that is not
    wanted gets a guarded buffer that is not passed; a sixth entry holds the workspace's dots_t, g_dots and g_dots_t
    (None where the call had no reason to write the region, which must then still hold the sentinel)."""
    dev = torch.device(device)
    mv = lambda t: None if t is None else t.to(dev).contiguous()                        # noqa: E731
    q, k, v, pos_src, pos_qry, inv_freq, weights, g = (mv(t) for t in (q, k, v, pos_src, pos_qry, inv_freq, weights, g))
    d = desc_of(cfg)
    assert lib.attn_path(d) == route_of(cfg["d"])
    nbytes = lib.attn_workspace_bytes(d)
    assert nbytes == 4 * cfg["batch"] * cfg["heads"] * cfg["d"] ** 2 * (max(chunks(cfg["n_src"]), chunks(cfg["n_qry"])) + 3)
    st = torch.cuda.current_stream().cuda_stream if dev.type == "cuda" else 0
    if guard:
        return _run_guarded(lib, cfg, dev, d, st, q, k, v, pos_src, pos_qry, inv_freq, rot_scale, weights, g, want)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
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


# ----------------------------------------------------------------------------------------------------------------------
# the kernel table: free-standing descriptors, each named after the edge it sits on (tests/test_gpu_attention_kernels.py
# runs all of them on the device, tests/test_emu_attention.py those with emu=True)
# ----------------------------------------------------------------------------------------------------------------------
VECTOR_D = (2, 4, 28, 30, 34, 36, 60, 62, 66, 68, 100, 124, 126)     # both ends of every lane layout DP = 32, 64, 128
MFMA_D = (32, 64, 128)
CHUNK_EDGES = (CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + TILE - 1, CHUNK + TILE + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1,
               8 * CHUNK + 1)                                         # the last: nine partials


def tile_edges(d):
    t = tile_of(d)
    return (t - 1, t, t + 1, 2 * t, 2 * t + 1)


def _kernel_cases():
    t = {}
    # lane layouts: every D next to a layout edge with every rotary form its descriptor allows, one past a tile
    for i, d in enumerate(VECTOR_D + MFMA_D):
        for r in (0, 1, 2):
            if r == 2 and d % 4:
                continue
            t[f"lanes_d{d}_rot{r}"] = desc_case(n_src=tile_of(d) + 1, d=d, rotary=r, heads=1 + (i + r) % 2,
                                                weights=(i + r) % 3 == 0,
                                                emu=(d, r) in ((30, 1), (34, 0), (36, 0), (100, 0), (100, 2), (32, 0), (64, 1),
                                                               (128, 0)))
    # h > 0 offsets, batches and weights on the widest layout of each route; H D = 300 is no multiple of 32
    t["lanes_d100_h3_b2_weights_no_rotary"] = desc_case(batch=2, n_src=TILE + 1, heads=3, d=100, rotary=0, weights=True)
    t["lanes_d124_h3_b2_weights_rot2"] = desc_case(batch=2, n_src=TILE + 1, heads=3, d=124, rotary=2, weights=True)
    t["lanes_d128_h3_b2_weights_no_rotary"] = desc_case(batch=2, n_src=65, heads=3, d=128, rotary=0, weights=True)
    t["lanes_d128_h3_b2_weights_rot1"] = desc_case(batch=2, n_src=65, heads=3, d=128, rotary=1, weights=True)
    t["lanes_d12_h3_hd36_signed_weights"] = desc_case(batch=2, n_src=TILE + 1, heads=3, d=12, rotary=0, weights="signed",
                                                      emu=True)
    # per-point tiles: T - 1, T, T + 1, 2 T, 2 T + 1 of k_attn_apply and k_attn_kv_bwd[_mfma]
    for d in (12,) + MFMA_D:
        for j, n in enumerate(tile_edges(d)):
            t[f"tile_d{d}_n{n}"] = desc_case(n_src=n, d=d, rotary=(0, 2, 0, 1, 0)[j], heads=2 if d < 128 else 1,
                                             emu=d == 12 or j == 2)
    # one, two and three points on every DP of both routes (the K-step is two points; D = 32 gives a wave eight)
    for d in (12, 36, 100) + MFMA_D:
        for n in (1, 2, 3):
            t[f"points_d{d}_n{n}"] = desc_case(n_src=n, d=d, rotary=(0, 2, 0, 1)[n], heads=2, batch=2, emu=True)
    # chunks of k_attn_outer / k_attn_reduce
    for d in (4, 32):
        for j, n in enumerate(CHUNK_EDGES):
            t[f"chunk_d{d}_n{n}"] = desc_case(n_src=n, d=d, rotary=(0, 2, 1)[j % 3], heads=2, weights=j % 2 == 1,
                                              emu=j < 3 and (d == 4 or j == 2))
    # the two sides in different chunk counts: the partials region is sized by the larger side
    for d in (12, 32, 128):
        t[f"cross_600_to_40_d{d}"] = desc_case(n_src=600, n_qry=40, d=d, rotary=0, heads=2 if d < 128 else 1,
                                               emu=d < 128)
        t[f"cross_40_to_600_d{d}_weights"] = desc_case(n_src=40, n_qry=600, d=d, rotary=2 if d == 12 else 0,
                                                       heads=2 if d < 128 else 1, weights=True, emu=d < 128)
    # marked points: g (q) is zero except at one query row, at the tile edges of the per-point kernels
    for d in (12, 32, 128):
        T = tile_of(d)
        n = 2 * T + 1
        for r in (0, T - 1, T, n - 1):
            t[f"marked_g_d{d}_n{n}_row{r}"] = desc_case(n_src=n, d=d, rotary=0, heads=2 if d < 128 else 1, mark_g=r,
                                                        emu=True)
        t[f"marked_q_d{d}_n{n}_row{T}"] = desc_case(n_src=n, d=d, rotary=0, heads=2 if d < 128 else 1, mark_q=T,
                                                    emu=True)
    t["zero_point_d64_one_chunk"] = desc_case(n_src=50, d=64, rotary=1, heads=2, zero_point=7, emu=True)
    t["constant_row_d12_no_rotary"] = desc_case(n_src=TILE + 2, d=12, rotary=0, heads=2, const_row=5, emu=True)
    return t


ATTN_KERNEL_CASES = _kernel_cases()
assert all(c["batch"] * max(c["n_src"], c["n_qry"]) * c["heads"] * c["d"] <= 2_000_000 for c in ATTN_KERNEL_CASES.values())
# one case per backward kernel instantiation at n = T + 1: all seven non-empty subsets of (gq, gk, gv) run on it
WANT_CASES = {"k_attn_kv_bwd<32>": "tile_d12_n33", "k_attn_kv_bwd<64>": "lanes_d36_rot0", "k_attn_kv_bwd<128>": "lanes_d100_rot0",
              "k_attn_kv_bwd_mfma<32>": "tile_d32_n129", "k_attn_kv_bwd_mfma<64>": "tile_d64_n129",
              "k_attn_kv_bwd_mfma<128>": "tile_d128_n65"}
WANT_SUBSETS = [tuple(bool(m >> i & 1) for i in range(3)) for m in range(1, 8)]
KERNEL_SEED = 47
TENSORS = ("u", "dots", "gq", "gk", "gv", "dots_t", "g_dots", "g_dots_t")
# the kernel that writes each checked tensor, by route, for the worst-ratio report
KERNEL_OF = {"u": "k_attn_apply mode 0", "dots": "k_attn_outer mode 0 + k_attn_reduce", "gq": "k_attn_apply mode 1",
             "gk": "k_attn_kv_bwd", "gv": "k_attn_kv_bwd", "dots_t": "k_attn_transpose",
             "g_dots": "k_attn_outer mode 1 + k_attn_reduce", "g_dots_t": "k_attn_reduce (transpose)"}
_REFERENCES = {}


def kernel_reference(name):
    """(inputs, {tensor: (value, A, N)}) of a kernel-table case, computed once and shared"""
    if name not in _REFERENCES:
        cfg = ATTN_KERNEL_CASES[name]
        args = desc_inputs(cfg, KERNEL_SEED)
        _REFERENCES[name] = (args, reference_with_bounds(cfg, args))
    return _REFERENCES[name]


def run_kernel_case(lib, name, device="cpu", want=(True, True, True)):
    """a kernel-table case through the C-ABI on guarded buffers at levels 1 and 2, with the exact zeros of its marks:
    ({tensor: value on the host or None}, {tensor: (rel-L2, row ratio, element ratio or None)})"""
    cfg = ATTN_KERNEL_CASES[name]
    args, ref = kernel_reference(name)
    got = run_descriptor(lib, cfg, *args, want=want, device=device, guard=True)
    named = dict(zip(TENSORS[:5], got[:5]))
    named.update(got[5])
    stats = check_levels(name, cfg, named, ref)
    for key, out in (("mark_g", "gq"), ("mark_q", "u")):
        r = cfg[key]
        if r is not None and named[out] is not None:         # every other query row is exactly zero
            others = [i for i in range(cfg["n_qry"]) if i != r]
            assert float(named[out][:, others].abs().max()) == 0.0 and float(named[out][:, r].abs().max()) > 0.0, name
    if cfg["mark_g"] is not None and named["g_dots"] is not None:          # g_dots is that row's outer product alone
        q, g, w = args[0].double(), args[8].double(), args[7]
        B, H, D, r = cfg["batch"], cfg["heads"], cfg["d"], cfg["mark_g"]
        wr = 1.0 / cfg["n_src"] if w is None else w.double()[:, r].reshape(B, 1, 1)
        outer = torch.einsum("bhi,bhj->bhij", q[:, r].reshape(B, H, D), g[:, r].reshape(B, H, D) * wr)
        assert cfg["rotary"] == 0 and rel_l2(outer.numpy(), ref["g_dots"][0].numpy()) < 1e-14
    return named, stats
