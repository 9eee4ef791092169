"""float64 restatement of the pointwise half of an FNO block (csrc/sc_kernels_pmlp.h, csrc/sc_kernels_plinx.h) for the
tests: the formulas, runners that drive the C-ABI on NaN-filled (and, on request, guarded) outputs, the constants of the
launch geometry read off the source, the case tables both tiers share, and per-element error bounds derived from the
kernels' arithmetic.  torch on the host; the engine is imported inside the runners only.

  MLP pass      out = act(W2 gelu(W1 x + b1) + b2 + gate (.) skip)               k_pmlp_fwd / k_pmlp_bwd
  block pass    s = conv + (Ws x + bs), y = act(s), out = MLP pass(y, skip = x)    k_pblock_fwd / k_pmlp_bwd<.., LIN>
  1 x 1 map     out = W x + b                                                      k_plin_fwd / k_plin_bwd
  plinx         out = act(W xin + b + gate (.) skip), xin = x or gelu(x), and its backward with PRO / XGRAD / addend
                                                                                   k_plinx_fwd / k_plinx_bwd

Bounds.  Every compared element must satisfy |got - want64| <= bound with no margin.  A value is carried as a pair
(v, e): v the float64 result, e a bound on |computed - v|.  A product chain of K terms on the matrix cores is charged two
roundings per term (v_mfma_f32_32x32x2_f32 is not documented to fuse) plus its bias / gate / skip additions; a sum over
pixels is charged the height of the tree the kernels really add along (tree_heights below); the activation is charged
the 1.5e-7 of A&S 7.1.26 on erfc plus the roundings of sc_erfc_core counted in erfc_parts.  DESIGN 3.10 / 3.17 carry
the same counts in prose."""
import math

import numpy as np
import torch

from fdconv_reference import U, gamma, worst_ratio

NAN = float("nan")
SENTINEL = -3.0e33                                           # guard-band value: no kernel here produces it

# ---- launch geometry, read off the source ------------------------------------------------------------------------------
TILE = 32                  # pixels of one sample a wave owns (sc_kernels_pmlp.h, header: "a tile of 32 pixels")
TILES_PER_WG = 4           # tile = wg * 4 + w: four waves of 64 lanes per workgroup (k_pmlp_fwd tile loop; NW = 4 backward)
PMLP_FWD_CAP = 2048        # sc_engine.cpp sc_pointwise_mlp_forward: `resident = wgs_env > 0 ? wgs_env : 2048`
PBLOCK_FWD_CAP = 2048      # sc_engine.cpp sc_pointwise_block_forward: `cap = wgs_env > 0 ? wgs_env : 2048`
PMLP_BWD_CAP = 256         # sc_engine.cpp pmlp_bwd_wgs: `cap = ... : 256` (one workgroup per CU); also the block backward
PLIN_BWD_CAP = 512         # sc_engine.cpp plin_bwd_wgs: `cap = env > 0 ? env : 512`
RED_GROUPS = 16            # sc_engine.cpp `#define SC_PMLP_RED_GROUPS 16`
WS_SLACK = 256             # every *_workspace_bytes ends in `* sizeof(float) + 256`
ACT_NONE, ACT_GELU, ACT_DGRAD = 0, 1, 2                      # include/sc_engine.h SC_ACT_NONE / SC_ACT_GELU / SC_ACT_GELU_DGRAD
XACT, ACT, PRO, XGRAD = 1, 2, 4, 8                           # sc_kernels_plinx.h SC_PLX_XACT / ACT / PRO / XGRAD


def cu_count(device):
    """what sc_cu_count() returns: the device's compute units, 1 in host emulation"""
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.device(device).type == "cuda" else 1


def plin_fwd_cap(c, cus):
    """sc_pointwise_linear_forward: per_cu = clamp(160 KB / lds, 1, 2) with lds = CI * 16 * CO * 64 * 4 + c_out * 4"""
    lds = (c // 32) * 16 * (c // 32) * 64 * 4 + c * 4
    return min(2, max(1, 160 * 1024 // lds)) * cus


def plinx_fwd_cap(cus):
    return 2 * cus                                           # sc_pointwise_linear_forward_ex: `resident = 2 * sc_cu_count()`


def plinx_omn(ci, co):
    """output tiles of 32 rows one launch of k_plinx_bwd owns (sc_engine.cpp plinx_omn: accumulator tiles <= 8)"""
    return min(co // 32, 8 // (ci // 32))


def plinx_bwd_cap(ci, co, lean, cus):
    """sc_kernels_plinx.h SC_PLX_BWD_OCC: two workgroups per unit for the LEAN kernel where CI * OMN <= 4, else one"""
    return (2 if lean and (ci // 32) * plinx_omn(ci, co) <= 4 else 1) * cus


def pmlp_np(ci, ch, co):
    """PmlpDims::NP: gw2 | gw1 | gb1 | gb2 | ggate"""
    return co * ch + ch * ci + ch + 2 * co


def plin_np(c):
    return c * c + c                                         # launch_plin_bwd: NP = NPW + 32 CO


def plinx_np(ci, co):
    omn = plinx_omn(ci, co)
    return omn * 32 * ci + 2 * omn * 32                      # PlinxDims::NP


def n_wg_from_workspace(nbytes, np_floats):
    """inverse of (n_wg + 16) * NP * 4 + 256"""
    q, r = divmod(nbytes - WS_SLACK, 4 * np_floats)
    assert r == 0 and q > RED_GROUPS, (nbytes, np_floats)
    return q - RED_GROUPS


def n_wg_for(tiles, cap):
    return min(-(-tiles // TILES_PER_WG), cap)


def shape_of_tiles(t):
    """(B, S) with B * S / 32 == t: B = 5 or 3 where t factors (an odd number of tiles per sample), else one sample"""
    named = {1: (1, 32), 3: (3, 32), 5: (5, 32), 15: (5, 96), 9: (3, 96)}
    if t in named:
        return named[t]
    for b in (5, 3):
        if t % b == 0:
            return b, 32 * (t // b)
    return 1, 32 * t


def second_round_tiles(cap, factor=True):
    """the smallest T >= 4 cap + 1 that factors by 3 or 5"""
    t = 4 * cap + 1
    while factor and t % 3 and t % 5:
        t += 1
    return t


# ---- float64 activation and the error of the engine's ------------------------------------------------------------------
_R2 = math.sqrt(2.0)
_AS = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)    # sc_erfc_core, A&S 7.1.26
_ASP = 0.3275911
AS_ERR = 1.5e-7                                              # |erfc - its A&S 7.1.26 form| (absolute), sc_device.h


def gelu64(v):
    return 0.5 * v * torch.special.erfc(-v / _R2)            # erfc: the negative tail does not cancel


def dgelu64(v):
    return 0.5 * torch.special.erfc(-v / _R2) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def erfc_parts(v):
    """(q, e, err_q, err_e): q = erfc(|v| / sqrt 2), e = exp(-v^2 / 2) and bounds on the error of what sc_erfc_core
    returns for them.  Counted in sc_device.h:
      t     the constant P rounded (1), fmaf(|v|, P, 1) (1), the reciprocal (rcp + one Newton step: 1 ulp = 2 u on the
            device; one division in emulation): relative 4 u
      p t   four fmaf and one product (5) on coefficients rounded to fp32 (5): gamma_10 on sum |a_i| t^i; the error of t
            enters through sum i |a_i| t^i
      e     (v v) E: two products and the constant (3 roundings of the exponent: relative 3 u s ln 2 on e) and exp2 itself
            (v_exp_f32: 1 ulp = 2 u; results below 2^-126 may flush to zero)
      q     (p t) e: one more product"""
    a = v.abs()
    t = 1.0 / (1.0 + (_ASP / _R2) * a)
    at, adt, tp = torch.zeros_like(t), torch.zeros_like(t), torch.ones_like(t)
    for i, c in enumerate(_AS, 1):
        tp = tp * t
        at += abs(c) * tp
        adt += i * abs(c) * tp
    e = torch.exp(-0.5 * v * v)
    q = torch.special.erfc(a / _R2)
    err_pt = gamma(10) * at + gamma(4) * adt
    rel_e = gamma(3) * (0.5 * v * v) + 2 * U                 # s ln 2 = v^2 / 2
    err_e = e * rel_e + 2.0 ** -126
    err_q = AS_ERR + e * err_pt * (1.0 + rel_e) + (q + AS_ERR) * rel_e + 2.0 ** -126 + U * (q + AS_ERR)
    return q, e, err_q, err_e


_ERR_PT = [abs(c) * (gamma(10) + i * gamma(4)) for i, c in enumerate(_AS, 1)]    # err_pt of erfc_parts as one polynomial in t
_DPHI = 1.0 / math.sqrt(2.0 * math.pi)


def act_parts(v):
    """(gelu, gelu_err, dgelu, dgelu_err) of float64 v from one evaluation of erfc and exp (the large cases spend their
    host time here).  The bounds are those of erfc_parts, for an exact fp32 argument:
      gelu_err   0.5 |v| (err_q + the rounding of fmaf(-cs, q, 1 + cs)) + the rounding of the product v h2
      dgelu_err  the same h2, D e (the constant and the product: 2 roundings on top of the error of e), the closing fmaf"""
    a, x2 = v.abs(), 0.5 * v * v
    t = 1.0 / (1.0 + (_ASP / _R2) * a)
    err_pt = torch.full_like(t, _ERR_PT[4])
    for c in reversed(_ERR_PT[:4]):
        err_pt.mul_(t).add_(c)
    err_pt.mul_(t)
    e = torch.exp(-x2)
    q = torch.special.erfc(a / _R2)
    rel_e = x2.mul_(gamma(3)).add_(2 * U)
    err_q = err_pt.mul_(e).mul_(1.0 + rel_e).add_((q + AS_ERR) * (rel_e + U)).add_(AS_ERR + 2.0 ** -126)
    w = torch.where(v < 0, q, 2.0 - q)
    half = err_q.add_(U * w).mul_(0.5)                       # error of h2 = w / 2
    g = 0.5 * v * w
    d = 0.5 * w + v * e * _DPHI
    err_e = rel_e.mul_(e).add_(2.0 ** -126).add_(gamma(2) * e)
    return g, half * a + U * g.abs(), d, half + a * err_e.mul_(_DPHI) + U * d.abs()


def gelu_err(v):
    """bound on |sc_gelu(v) - gelu(v)| for an exact fp32 argument"""
    return act_parts(v)[1]


def dgelu_err(v):
    """bound on |sc_gelu_both's derivative - (Phi + v phi)| for an exact fp32 argument"""
    return act_parts(v)[3]


GELU_LIP, DGELU_LIP = 1.13, 0.8                              # sup |gelu'| = 1.1290, sup |gelu''| = 2 phi(0) = 0.7979


class V:
    """v: float64 value; e: bound on |what the kernel computed - v|"""
    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e

    @property
    def mag(self):
        return self.v.abs() + self.e


def _d(t):
    return None if t is None else t.detach().double().cpu()


def _vec(b):
    return 0.0 if b is None else b[None, :, None]


def v_act(x):
    """(gelu, gelu') of a carried value"""
    g, ge, d, de = act_parts(x.v)
    return V(g, ge.add_(GELU_LIP * x.e)), V(d, de.add_(DGELU_LIP * x.e))


def v_gelu(x):
    return v_act(x)[0]


def v_dgelu(x):
    return v_act(x)[1]


def v_mul(a, b):
    """one rounded product of two carried values"""
    return V(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e + U * a.mag * b.mag)


def v_map(w, x, adds=(), n_extra=0, transpose=False):
    """sum_c w[o, c] x[b, c, s] (+ exact addends) on the matrix cores: two roundings per term of the K extent plus one per
    addend (a fused multiply-add of gate and skip counts one).  adds: (value, magnitude) float64 pairs, exact inputs."""
    eq = "oc,bos->bcs" if transpose else "oc,bcs->bos"
    k = w.shape[0] if transpose else w.shape[1]
    val = torch.einsum(eq, w, x.v)
    a = torch.einsum(eq, w.abs(), x.mag)
    err = torch.einsum(eq, w.abs(), x.e) if bool((x.e != 0).any()) else torch.zeros_like(val)
    for v, m in adds:
        val = val + v
        a = a + m
    return V(val, err + gamma(2 * k + len(adds) + n_extra) * a)


def tree_heights(tiles, n_wg):
    """(H_w, H_s): roundings on the longest path of a sum over all pixels.
      rounds  tiles a wave takes: ceil(T / (4 n_wg))
      H_w     weight gradients: 32 pixels per tile on the matrix cores (2 roundings each) per round, the four waves' turns
              into the LDS image, ceil(n_wg / groups) additions in k_pmlp_reduce1, `groups` in the final stage
      H_s     bias / gate gradients: a lane adds 16 pixels per tile one after the other (17 for k_plinx_bwd's ggate, which
              sums a tile first), two half rows x four waves into the LDS image, then the same two stages"""
    rounds = -(-tiles // (TILES_PER_WG * n_wg))
    groups = min(n_wg, RED_GROUPS)
    stages = -(-n_wg // groups) + groups
    return 2 * TILE * rounds + 4 + stages, 17 * rounds + 8 + stages


def v_outer(g, x, h):
    """sum over (batch, pixel) of g[b, o, s] x[b, c, s] along a tree of height h"""
    val = torch.einsum("bos,bcs->oc", g.v, x.v)
    a = torch.einsum("bos,bcs->oc", g.mag, x.mag)
    err = torch.einsum("bos,bcs->oc", g.mag, x.e) + torch.einsum("bos,bcs->oc", g.e, x.v.abs())
    return V(val, err + gamma(h) * a)


def v_rowsum(g, h):
    return V(g.v.sum((0, 2)), g.e.sum((0, 2)) + gamma(h) * g.mag.sum((0, 2)))


# ---- references: dict name -> V -----------------------------------------------------------------------------------------
def ref_mlp_forward(inp, act, x=None):
    """the MLP pass; x: a carried input (the block pass hands y over with its error)"""
    w1, b1, w2, b2 = (_d(inp[k]) for k in ("w1", "b1", "w2", "b2"))
    x = V(_d(inp["x"])) if x is None else x
    gated = inp.get("gate") is not None
    hp = v_map(w1, x, adds=[] if b1 is None else [(_vec(b1), _vec(b1).abs())], n_extra=0 if b1 is not None else 1)
    h, dh = v_act(hp)
    adds = [(_vec(b2), _vec(b2).abs())] if b2 is not None else [(0.0, 0.0)]
    if gated:
        gs = _vec(_d(inp["gate"])) * _d(inp["skip"])
        adds.append((gs, gs.abs()))
    z = v_map(w2, h, adds=adds)
    return dict(hp=hp, h=h, dh=dh, z=z, out=v_gelu(z) if act else z)


def ref_block_forward(inp, act):
    """s / y / out (and the stored derivative) of k_pblock_fwd; the gated skip of its MLP is the block input x"""
    ws, bs = _d(inp["ws"]), _d(inp["bs"])
    x, conv = _d(inp["x"]), _d(inp["conv"])
    s = v_map(ws, V(x), adds=[(_vec(bs), abs(_vec(bs)) if bs is None else _vec(bs).abs()), (conv, conv.abs())])
    y, ds = v_act(s) if act else (s, None)
    mlp = ref_mlp_forward(dict(inp, skip=inp["x"]), 1 if act else 0, x=y)
    out = dict(y=y, out=mlp["out"])
    if act:
        out["pre"] = ds if act == ACT_DGRAD else s
    return out


def ref_mlp_backward(inp, act, tiles, n_wg, xpre=None, lin=False):
    """every gradient of k_pmlp_bwd.  act: the MLP's closing activation (0 / 1); xpre: None, "pre" (x = gelu(x_pre): gx is
    taken through gelu'(x_pre)) or "grad" (x_pre holds that derivative); lin: gskip = W_s^T gx + gate (.) gz"""
    hw, hs = tree_heights(tiles, n_wg)
    fw = ref_mlp_forward(inp, 0)
    w1, w2 = _d(inp["w1"]), _d(inp["w2"])
    x, gout = V(_d(inp["x"])), V(_d(inp["gout"]))
    gated = inp.get("gate") is not None
    gz = v_mul(gout, v_dgelu(fw["z"])) if act else gout
    res = {}
    if gated:
        gate, skip = V(_vec(_d(inp["gate"])) + torch.zeros(1, 1, 1, dtype=torch.float64)), V(_d(inp["skip"]))
        gk = v_mul(gate, gz)
        if not lin:
            res["gskip"] = gk
        res["ggate"] = v_rowsum(v_mul(gz, skip), hs)
    res["gb2"] = v_rowsum(gz, hs)
    res["gw2"] = v_outer(gz, fw["h"], hw)
    gh = v_map(w2, gz, transpose=True)
    ghp = v_mul(gh, fw["dh"])
    res["gb1"] = v_rowsum(ghp, hs)
    res["gw1"] = v_outer(ghp, x, hw)
    gx = v_map(w1, ghp, transpose=True)
    if xpre == "pre":
        gx = v_mul(gx, v_dgelu(V(_d(inp["x_pre"]))))
    elif xpre == "grad":
        gx = v_mul(gx, V(_d(inp["x_pre"])))
    res["gx"] = gx
    if lin:
        res["gin"] = v_map(_d(inp["ws"]), gx, adds=[(gk.v, gk.mag)], transpose=True)
        res["gin"].e = res["gin"].e + gk.e
    return res


def ref_linear(inp, tiles=None, n_wg=None):
    """the 1 x 1 map and, with gout, its backward (gx = W^T g + addend, gw, gb)"""
    w, b, x = _d(inp["w"]), _d(inp.get("bias")), V(_d(inp["x"]))
    res = dict(out=v_map(w, x, adds=[(_vec(b), abs(_vec(b)) if b is None else _vec(b).abs())]))
    if inp.get("gout") is not None:
        hw, hs = tree_heights(tiles, n_wg)
        g, add = V(_d(inp["gout"])), _d(inp.get("addend"))
        res["gx"] = v_map(w, g, adds=[] if add is None else [(add, add.abs())], transpose=True)
        res["gw"] = v_outer(g, x, hw)
        res["gb"] = v_rowsum(g, hs)
    return res


def ref_plinx_forward(inp, flags):
    w, b, x = _d(inp["w"]), _d(inp.get("bias")), V(_d(inp["x"]))
    xin = v_gelu(x) if flags & XACT else x
    adds = [(_vec(b), abs(_vec(b)) if b is None else _vec(b).abs())]
    if inp.get("gate") is not None:
        gs = _vec(_d(inp["gate"])) * _d(inp["skip"])
        adds.append((gs, gs.abs()))
    z = v_map(w, xin, adds=adds)
    return dict(pre=z, out=v_gelu(z) if flags & ACT else z)


def ref_plinx_backward(inp, flags, tiles, n_wg):
    """g = gout (.) gelu'(pre) (PRO); gskip = gate (.) g, ggate; gx = (W^T g + addend) (.) gelu'(xg) (XGRAD);
    gw = g xin^T with xin = gelu(x) (XACT); gb = sum g"""
    hw, hs = tree_heights(tiles, n_wg)
    w, x = _d(inp["w"]), V(_d(inp["x"]))
    g = V(_d(inp["gout"]))
    if flags & PRO:
        g = v_mul(g, v_dgelu(V(_d(inp["pre"]))))
    res = {}
    if inp.get("gate") is not None:
        res["gskip"] = v_mul(V(_vec(_d(inp["gate"])) + torch.zeros(1, 1, 1, dtype=torch.float64)), g)
        res["ggate"] = v_rowsum(v_mul(g, V(_d(inp["skip"]))), hs)
    add = _d(inp.get("addend"))
    gx = v_map(w, g, adds=[] if add is None else [(add, add.abs())], transpose=True)
    if flags & XGRAD:
        gx = v_mul(gx, v_dgelu(V(_d(inp["xg"]))))
    res["gx"] = gx
    res["gw"] = v_outer(g, v_gelu(x) if flags & XACT else x, hw)
    res["gb"] = v_rowsum(g, hs)
    return res


# ---- comparison -----------------------------------------------------------------------------------------------------------
def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def worst_ratio_large(got, want, bound):
    """fdconv_reference.worst_ratio on torch tensors (threaded: the largest cases hold 3e7 elements): max |got - want| /
    bound; where bound == 0 the value must be exactly 0 (inf if not)"""
    zero = bound == 0
    if bool((zero & (got != 0)).any()) or not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - want).abs_() / torch.where(zero, torch.ones_like(bound), bound)).max())


def check(tag, got, want, tol):
    """got / want: dicts by tensor name (got: host fp32 tensors, want: V).  Every tensor of `got` meets rel-L2 `tol` and,
    per element, |got - want| <= bound (ratio <= 1; where the bound is 0 the value is exactly 0).  Returns the ratios."""
    ratios, errs = {}, {}
    for k, t in got.items():
        if t is None:
            continue
        w = want[k]
        assert tuple(t.shape) == tuple(w.v.shape) or t.numel() == w.v.numel(), (tag, k, t.shape, w.v.shape)
        gt = t.double().reshape(w.v.shape)
        if gt.numel() < 1 << 20:
            ratios[k] = worst_ratio(gt.numpy(), w.v.numpy(), (w.e / gamma(1)).numpy(), 1)
        else:
            ratios[k] = worst_ratio_large(gt, w.v, w.e)
        nrm = float(torch.linalg.vector_norm(w.v))
        errs[k] = float(torch.linalg.vector_norm(gt - w.v)) / nrm if nrm > 0 else float(gt.abs().max())
    print(tag, "ratio", {k: f"{r:.3f}" for k, r in ratios.items()}, "rel-L2", {k: f"{e:.1e}" for k, e in errs.items()})
    for k in ratios:
        assert errs[k] < tol, (tag, k, errs[k], tol)
        assert ratios[k] <= 1.0, (tag, k, ratios[k])
    return ratios


# ---- guarded storage -----------------------------------------------------------------------------------------------------
class Guarded:
    """a NaN-filled tensor inside a larger allocation: `pad` floats of SENTINEL before and after it"""
    def __init__(self, shape, pad, device):
        n = int(np.prod(shape))
        self.pad = pad
        self.full = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.float32, device=device)
        self.t = self.full[pad:pad + n].view(*shape)
        self.t.fill_(NAN)

    def assert_intact(self, name, written=True):
        lo, hi = self.full[:self.pad], self.full[self.pad + self.t.numel():]
        assert bool((lo == SENTINEL).all()) and bool((hi == SENTINEL).all()), name + ": a guard band was written"
        if written:
            assert not bool(torch.isnan(self.t).any()), name + ": an element was left unwritten"
        else:
            assert bool(torch.isnan(self.t).all()), name + ": an unwanted tensor was written"


class _Outputs:
    """NaN-filled outputs by name; with guard, each inside its own guarded allocation"""
    def __init__(self, device, guard):
        self.device, self.guard, self.g, self.t = device, guard, {}, {}

    def new(self, name, shape, pad=None):
        if self.guard:
            pad = int(np.prod(shape[1:])) if pad is None else pad
            self.g[name] = Guarded(shape, max(pad, 1024), self.device)
            self.t[name] = self.g[name].t
        else:
            self.t[name] = torch.full(tuple(shape), NAN, dtype=torch.float32, device=self.device)
        return self.t[name].data_ptr()

    def workspace(self, nbytes, np_floats):
        """exactly nbytes, followed by at least NP floats of sentinel when guarded"""
        assert nbytes > 0 and nbytes % 4 == 0
        tail = max(np_floats, 1024) if self.guard else 0
        self.ws = torch.full((nbytes // 4 + tail,), SENTINEL, dtype=torch.float32, device=self.device)
        self.ws_floats = nbytes // 4
        return self.ws.data_ptr()

    def finish(self, unwanted=()):
        if self.device != "cpu" and torch.device(self.device).type == "cuda":
            torch.cuda.synchronize()
        for k, g in self.g.items():
            g.assert_intact(k, written=k not in unwanted)
        if self.guard and hasattr(self, "ws"):
            assert bool((self.ws[self.ws_floats:] == SENTINEL).all()), "the workspace was overrun"
        return {k: (None if k in unwanted else t.cpu()) for k, t in self.t.items()}


def _p(t):
    return 0 if t is None else t.data_ptr()


def _to(inp, device):
    return {k: (None if v is None else v.to(device).contiguous()) for k, v in inp.items() if torch.is_tensor(v) or v is None}


# ---- runners: (lib, cfg, inputs on the host) -> outputs on the host ------------------------------------------------------
def run_mlp_forward(lib, cfg, inp, device="cpu", stream=0, guard=False):
    (ci, ch, co), B, S = cfg["chans"], cfg["B"], cfg["S"]
    d, o = _to(inp, device), _Outputs(device, guard)
    lib.pointwise_mlp_forward(B, ci, ch, co, S, cfg["act"], _p(d["x"]), _p(d["w1"]), _p(d.get("b1")), _p(d["w2"]), _p(d.get("b2")),
                              _p(d.get("skip")), _p(d.get("gate")), o.new("out", (B, co, S)), stream)
    return o.finish()


def run_block_forward(lib, cfg, inp, device="cpu", stream=0, guard=False):
    (c, ch), B, S, act = cfg["chans"], cfg["B"], cfg["S"], cfg["act"]
    d, o = _to(inp, device), _Outputs(device, guard)
    y, pre, out = o.new("y", (B, c, S)), (o.new("pre", (B, c, S)) if act else 0), o.new("out", (B, c, S))
    lib.pointwise_block_forward(B, c, ch, S, act, _p(d["conv"]), _p(d["x"]), _p(d["ws"]), _p(d.get("bs")), _p(d["w1"]), _p(d.get("b1")),
                                _p(d["w2"]), _p(d.get("b2")), _p(d["gate"]), y, pre, out, stream)
    return o.finish()


def mlp_backward_n_wg(lib, cfg):
    (ci, ch, co), B, S = cfg["chans"], cfg["B"], cfg["S"]
    return n_wg_from_workspace(lib.pointwise_mlp_workspace_bytes(B, ci, ch, co, S, 1), pmlp_np(ci, ch, co))


def run_mlp_backward(lib, cfg, inp, device="cpu", stream=0, guard=False):
    """sc_pointwise_mlp_backward_ex; cfg: chans, B, S, act (0 / 1), gate, xpre (None / "pre" / "grad"), gbias"""
    (ci, ch, co), B, S = cfg["chans"], cfg["B"], cfg["S"]
    d, o = _to(inp, device), _Outputs(device, guard)
    act = ACT_DGRAD if cfg["xpre"] == "grad" else (ACT_GELU if cfg["act"] else ACT_NONE)
    gated, gbias = d.get("gate") is not None, cfg.get("gbias", True) and d.get("b1") is not None
    gx, gw1, gw2 = o.new("gx", (B, ci, S)), o.new("gw1", (ch, ci), 0), o.new("gw2", (co, ch), 0)
    gb1, gb2 = o.new("gb1", (ch,), 0), o.new("gb2", (co,), 0)          # a NaN-filled dummy stays untouched when not wanted
    gsk = o.new("gskip", (B, co, S)) if gated else 0
    ggt = o.new("ggate", (co,), 0)
    ws = o.workspace(lib.pointwise_mlp_workspace_bytes(B, ci, ch, co, S, act), pmlp_np(ci, ch, co))
    lib.pointwise_mlp_backward(B, ci, ch, co, S, act, _p(d["x"]), _p(d["w1"]), _p(d.get("b1")), _p(d["w2"]), _p(d.get("b2")),
                               _p(d.get("skip")), _p(d.get("gate")), _p(d["gout"]), gx, gw1, gb1 if gbias else 0, gw2,
                               gb2 if gbias else 0, gsk, ggt if gated else 0, ws, stream, x_pre=_p(d.get("x_pre")))
    return o.finish(unwanted=(() if gbias else ("gb1", "gb2")) + (() if gated else ("ggate",)))


def run_block_backward(lib, cfg, inp, device="cpu", stream=0, guard=False):
    """sc_pointwise_block_backward; inp: x (= y, the MLP's input), x_pre (y_pre), skip (the block input), ws, ..."""
    (c, ch), B, S, act = cfg["chans"], cfg["B"], cfg["S"], cfg["act"]
    d, o = _to(inp, device), _Outputs(device, guard)
    gz, gin = o.new("gx", (B, c, S)), o.new("gin", (B, c, S))
    gw1, gb1, gw2, gb2, ggt = (o.new(k, s, 0) for k, s in (("gw1", (ch, c)), ("gb1", (ch,)), ("gw2", (c, ch)), ("gb2", (c,)),
                                                          ("ggate", (c,))))
    ws = o.workspace(lib.pointwise_mlp_workspace_bytes(B, c, ch, c, S, 1), pmlp_np(c, ch, c))
    lib.pointwise_block_backward(B, c, ch, S, act, _p(d["x"]), _p(d.get("x_pre")), _p(d["skip"]), _p(d["ws"]), _p(d["w1"]), _p(d["b1"]),
                                 _p(d["w2"]), _p(d["b2"]), _p(d["gate"]), _p(d["gout"]), gz, gin, gw1, gb1, gw2, gb2, ggt, ws, stream)
    return o.finish()


def run_linear_forward(lib, cfg, inp, device="cpu", stream=0, guard=False):
    c, B, S = cfg["c"], cfg["B"], cfg["S"]
    d, o = _to(inp, device), _Outputs(device, guard)
    lib.pointwise_linear_forward(B, c, c, S, _p(d["x"]), _p(d["w"]), _p(d.get("bias")), o.new("out", (B, c, S)), stream)
    return o.finish()


def linear_backward_n_wg(lib, cfg):
    return n_wg_from_workspace(lib.pointwise_linear_workspace_bytes(cfg["B"], cfg["c"], cfg["c"], cfg["S"]), plin_np(cfg["c"]))


def run_linear_backward(lib, cfg, inp, device="cpu", stream=0, guard=False):
    c, B, S = cfg["c"], cfg["B"], cfg["S"]
    d, o = _to(inp, device), _Outputs(device, guard)
    gx, gw, gb = o.new("gx", (B, c, S)), o.new("gw", (c, c), 0), o.new("gb", (c,), 0)
    ws = o.workspace(lib.pointwise_linear_workspace_bytes(B, c, c, S), plin_np(c))
    want_gb = cfg.get("gbias", True)
    lib.pointwise_linear_backward(B, c, c, S, _p(d["x"]), _p(d["w"]), _p(d["gout"]), gx, gw, gb if want_gb else 0, ws, stream,
                                  addend=_p(d.get("addend")))
    return o.finish(unwanted=() if want_gb else ("gb",))


def run_plinx_forward(lib, cfg, inp, device="cpu", stream=0, guard=False):
    ci, co, B, S = cfg["ci"], cfg["co"], cfg["B"], cfg["S"]
    d, o = _to(inp, device), _Outputs(device, guard)
    out = o.new("out", (B, co, S))
    pre = o.new("pre", (B, co, S)) if cfg.get("pre_out", True) else 0
    lib.pointwise_linear_forward_ex(B, ci, co, S, cfg["flags"], _p(d["x"]), _p(d["w"]), _p(d.get("bias")), _p(d.get("skip")),
                                    _p(d.get("gate")), out, pre, stream)
    return o.finish()


def plinx_is_lean(cfg, inp):
    return not cfg.get("want_gx", True) and cfg["flags"] == 0 and inp.get("gate") is None


def plinx_backward_n_wg(lib, cfg, inp, cus):
    """the workspace is sized for the larger (LEAN) grid; the grid of this call follows plinx_bwd_wgs"""
    ci, co, B, S = cfg["ci"], cfg["co"], cfg["B"], cfg["S"]
    tiles = B * S // TILE
    big = n_wg_from_workspace(lib.pointwise_linear_workspace_bytes_ex(B, ci, co, S), plinx_np(ci, co))
    assert big == n_wg_for(tiles, plinx_bwd_cap(ci, co, True, cus)), (big, tiles, cus)
    return n_wg_for(tiles, plinx_bwd_cap(ci, co, plinx_is_lean(cfg, inp), cus))


def run_plinx_backward(lib, cfg, inp, device="cpu", stream=0, guard=False):
    """sc_pointwise_linear_backward_ex; cfg: ci, co, B, S, flags, want_gx"""
    ci, co, B, S = cfg["ci"], cfg["co"], cfg["B"], cfg["S"]
    d, o = _to(inp, device), _Outputs(device, guard)
    gated, want_gx = d.get("gate") is not None, cfg.get("want_gx", True)
    gx = o.new("gx", (B, ci, S)) if want_gx else 0
    gw, gb = o.new("gw", (co, ci), 0), o.new("gb", (co,), 0)
    gsk = o.new("gskip", (B, co, S)) if gated and want_gx else 0
    ggt = o.new("ggate", (co,), 0)
    ws = o.workspace(lib.pointwise_linear_workspace_bytes_ex(B, ci, co, S), plinx_np(ci, co))
    lib.pointwise_linear_backward_ex(B, ci, co, S, cfg["flags"], _p(d["x"]), _p(d["w"]), _p(d["gout"]), _p(d.get("pre")), _p(d.get("xg")),
                                     _p(d.get("skip")), _p(d.get("gate")), _p(d.get("addend")) if want_gx else 0, gx, gw, gb, gsk,
                                     ggt if gated else 0, ws, stream)
    return o.finish(unwanted=() if gated else ("ggate",))


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _gen(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s, sc=1.0: torch.randn(*s, generator=g) * sc


def mlp_inputs(cfg, seed, backward=False):
    (ci, ch, co), B, S = cfg["chans"], cfg["B"], cfg["S"]
    mk = _gen(seed)
    inp = dict(x=mk(B, ci, S), w1=mk(ch, ci, sc=ci ** -0.5), w2=mk(co, ch, sc=ch ** -0.5))
    inp["b1"], inp["b2"] = (mk(ch), mk(co)) if cfg.get("bias", True) else (None, None)
    inp["skip"], inp["gate"] = (mk(B, co, S), mk(co)) if cfg.get("gate", True) else (None, None)
    if backward:
        inp["gout"] = mk(B, co, S)
        if cfg.get("xpre"):                                   # x = gelu(x_pre) as the previous pass left it, fp32
            pre = inp["x"]
            inp["x"] = gelu64(pre.double()).float()
            inp["x_pre"] = dgelu64(pre.double()).float() if cfg["xpre"] == "grad" else pre
    return inp


def block_inputs(cfg, seed, backward=False):
    (c, ch), B, S, act = cfg["chans"], cfg["B"], cfg["S"], cfg["act"]
    mk = _gen(seed)
    bias = cfg.get("bias", True)
    inp = dict(x=mk(B, c, S), conv=mk(B, c, S), ws=mk(c, c, sc=c ** -0.5), w1=mk(ch, c, sc=c ** -0.5), w2=mk(c, ch, sc=ch ** -0.5),
               gate=mk(c))
    inp["bs"], inp["b1"], inp["b2"] = (mk(c), mk(ch), mk(c)) if bias else (None, None, None)
    if backward:                                             # the backward kernel's view: x = y, skip = the block input
        pre = inp.pop("conv")
        inp["skip"], inp["gout"] = inp["x"], mk(B, c, S)
        inp["x"] = gelu64(pre.double()).float() if act else pre
        inp["x_pre"] = None if not act else (dgelu64(pre.double()).float() if act == ACT_DGRAD else pre)
    return inp


def linear_inputs(cfg, seed, backward=False):
    c, B, S = cfg["c"], cfg["B"], cfg["S"]
    mk = _gen(seed)
    inp = dict(x=mk(B, c, S), w=mk(c, c, sc=c ** -0.5), bias=mk(c) if cfg.get("bias", True) else None)
    if backward:
        inp["bias"] = None
        inp["gout"] = mk(B, c, S)
        inp["addend"] = mk(B, c, S) if cfg.get("addend") else None
    return inp


def plinx_inputs(cfg, seed, backward=False):
    ci, co, B, S, flags = cfg["ci"], cfg["co"], cfg["B"], cfg["S"], cfg["flags"]
    mk = _gen(seed)
    inp = dict(x=mk(B, ci, S), w=mk(co, ci, sc=ci ** -0.5))
    inp["skip"], inp["gate"] = (mk(B, co, S), mk(co)) if cfg.get("gated") else (None, None)
    if not backward:
        inp["bias"] = mk(co) if cfg.get("bias", True) else None
        return inp
    inp["gout"] = mk(B, co, S)
    inp["pre"] = mk(B, co, S) if flags & PRO else None
    inp["addend"] = mk(B, ci, S) if cfg.get("addend") and cfg.get("want_gx", True) else None
    inp["xg"] = inp["x"] if flags & XACT and flags & XGRAD else (mk(B, ci, S) if flags & XGRAD else None)
    return inp


def mark_tile(inp, tile, S, keys=("gout", "skip", "addend")):
    """zero gout (and skip, addend) everywhere but in one tile of 32 pixels"""
    out = dict(inp)
    b, px = divmod(tile, S // TILE)
    for k in keys:
        if out.get(k) is not None:
            t = torch.zeros_like(out[k])
            t[b, :, TILE * px:TILE * (px + 1)] = out[k][b, :, TILE * px:TILE * (px + 1)]
            out[k] = t
    return out


# ---- case tables -------------------------------------------------------------------------------------------------------------
A_TILES = (1, 3, 5, 15, 61, 65)
EMU_TILES = (1, 3, 5, 15)
MLP_SHAPES = {111: (32, 32, 32), 212: (64, 32, 64), 222: (64, 64, 64), 424: (128, 64, 128)}
PLX_CHANS = (32, 64, 128)


def _bs(t):
    b, s = shape_of_tiles(t)
    return dict(B=b, S=s, T=t)


def _mlp_fwd_cases():
    c, tiles = {}, list(A_TILES)
    for sid, chans in MLP_SHAPES.items():
        for i, (gate, act, bias) in enumerate([(g, a, b) for g in (1, 0) for a in (1, 0) for b in (1, 0)]):
            t = tiles[(i + sid) % len(tiles)]
            c[f"a_{sid}_g{gate}a{act}b{bias}_T{t}"] = dict(chans=chans, gate=gate, act=act, bias=bias, sid=sid, **_bs(t))
        for t in A_TILES:                                    # every tile count with everything on
            c[f"a_{sid}_g1a1b1_T{t}"] = dict(chans=chans, gate=1, act=1, bias=1, sid=sid, **_bs(t))
    return c


def _block_fwd_cases():
    c = {}
    for sid in (111, 212, 222):
        ci, ch, _ = MLP_SHAPES[sid]
        for i, (act, bias) in enumerate([(a, b) for a in (ACT_NONE, ACT_GELU, ACT_DGRAD) for b in (1, 0)]):
            t = A_TILES[(i + sid) % len(A_TILES)]
            c[f"a_{sid}_act{act}b{bias}_T{t}"] = dict(chans=(ci, ch), act=act, bias=bias, sid=sid, **_bs(t))
        for t in A_TILES:
            c[f"a_{sid}_act2b1_T{t}"] = dict(chans=(ci, ch), act=ACT_DGRAD, bias=1, sid=sid, **_bs(t))
    return c


def _mlp_bwd_cases():
    c = {}
    variants = [(g, a, xp, gb) for g in (1, 0) for a, xp in ((0, None), (0, "pre"), (1, None), (1, "pre"), (1, "grad")) for gb in (1, 0)]
    for sid in (111, 212, 222):
        for i, (gate, act, xp, gb) in enumerate(variants):
            t = A_TILES[(i + sid) % len(A_TILES)]
            c[f"a_{sid}_g{gate}a{act}x{xp or 'null'}gb{gb}_T{t}"] = dict(chans=MLP_SHAPES[sid], gate=gate, act=act, xpre=xp, gbias=gb,
                                                                         sid=sid, **_bs(t))
        for t in A_TILES:
            c[f"a_{sid}_g1a1xgradgb1_T{t}"] = dict(chans=MLP_SHAPES[sid], gate=1, act=1, xpre="grad", gbias=1, sid=sid, **_bs(t))
    return c


def _block_bwd_cases():
    c = {}
    for sid in (111, 212):
        ci, ch, _ = MLP_SHAPES[sid]
        for act in (ACT_NONE, ACT_GELU, ACT_DGRAD):
            for t in A_TILES if act == ACT_DGRAD else (A_TILES[(act + sid) % 6], 65):
                c[f"a_{sid}_act{act}_T{t}"] = dict(chans=(ci, ch), act=act, sid=sid, **_bs(t))
    return c


def _lin_cases():
    f, b = {}, {}
    for ch in (32, 64, 128):
        for bias in (1, 0):
            for t in A_TILES if bias else (5,):
                f[f"a_{ch}_b{bias}_T{t}"] = dict(c=ch, bias=bias, **_bs(t))
    for ch in (32, 64):
        for i, (add, gb) in enumerate([(1, 1), (0, 1), (1, 0), (0, 0)]):
            for t in A_TILES if i == 0 else (A_TILES[(i + ch // 32) % 6],):
                b[f"a_{ch}_add{add}gb{gb}_T{t}"] = dict(c=ch, addend=add, gbias=gb, **_bs(t))
    return f, b


PLX_BWD_VARIANTS = [(0, False, False), (XACT | XGRAD | PRO, True, False), (XGRAD, False, True), (PRO, True, True)]   # test_emu_plinx.test_backward


def _plinx_cases():
    f, b = {}, {}
    pairs = [(ci, co) for ci in PLX_CHANS for co in PLX_CHANS]
    for n, (ci, co) in enumerate(pairs):
        for i, (flags, gated, pre) in enumerate([(fl, g, p) for fl in (0, XACT, ACT, XACT | ACT) for g in (1, 0) for p in (1, 0)]):
            if (i + n) % 4 and not (flags == (XACT | ACT) and gated and pre):          # a quarter of the product, and all-on
                continue
            for t in A_TILES if (flags == (XACT | ACT) and gated and pre and ci == co) else (A_TILES[(i + n) % 6],):
                f[f"a_{ci}_{co}_f{flags}g{gated}p{pre}_T{t}"] = dict(ci=ci, co=co, flags=flags, gated=gated, pre_out=pre, **_bs(t))
        for i, (flags, gated, add) in enumerate(PLX_BWD_VARIANTS):
            for want_gx in (1, 0):
                fl = flags if want_gx else flags & ~XGRAD
                for t in A_TILES if (i == 1 and want_gx and ci == co) or (i == 0 and not want_gx and ci == co) else (A_TILES[(i + n + want_gx) % 6],):
                    b[f"a_{ci}_{co}_f{fl}g{int(gated)}add{int(add)}gx{want_gx}_T{t}"] = dict(ci=ci, co=co, flags=fl, gated=gated, addend=add,
                                                                                       want_gx=want_gx, **_bs(t))
    return f, b


MLP_FWD_KERNEL_CASES = _mlp_fwd_cases()
BLOCK_FWD_KERNEL_CASES = _block_fwd_cases()
MLP_BWD_KERNEL_CASES = _mlp_bwd_cases()
BLOCK_BWD_KERNEL_CASES = _block_bwd_cases()
LIN_FWD_KERNEL_CASES, LIN_BWD_KERNEL_CASES = _lin_cases()
PLINX_FWD_KERNEL_CASES, PLINX_BWD_KERNEL_CASES = _plinx_cases()


def emu_subset(table, key):
    """one case per `key` value at every tile count the emulated chip takes (T <= 15)"""
    seen, out = set(), []
    for name in sorted(table):
        cfg = table[name]
        k = (key(cfg), cfg["T"])
        if cfg["T"] in EMU_TILES and k not in seen:
            seen.add(k)
            out.append(name)
    return out


# ---- instantiations: the arms of the dispatchers in the pointwise section of sc_engine.cpp --------------------------------
def instantiation(kind, cfg, inp=None):
    if kind == "mlp_fwd":
        return f"k_pmlp_fwd<{cfg['sid']},{int(bool(cfg['gate']))},{cfg['act']}>"
    if kind == "block_fwd":
        return f"k_pblock_fwd<{cfg['sid']},{int(cfg['act'] != ACT_NONE)}>"
    if kind == "mlp_bwd":
        return f"k_pmlp_bwd<{cfg['sid']},{int(bool(cfg['gate']))},{cfg['act']}>"
    if kind == "block_bwd":
        return f"k_pmlp_bwd<{cfg['sid']},LIN,{int(cfg['act'] != ACT_NONE)}>"
    if kind in ("lin_fwd", "lin_bwd"):
        return f"k_plin_{kind[4:]}<{cfg['c'] // 32}{cfg['c'] // 32}>"
    if kind == "plinx_fwd":
        return f"k_plinx_fwd<{cfg['ci'] // 32}{cfg['co'] // 32}>"
    lean = not cfg["want_gx"] and cfg["flags"] == 0 and not cfg["gated"]
    return f"k_plinx_bwd<{cfg['ci'] // 32}{cfg['co'] // 32}{',LEAN' if lean else ''}>"


def dispatcher_arms():
    """every template instantiation a `switch` (or its if-chain) of the pointwise section can launch"""
    arms = set()
    for sid in (111, 212, 222, 424):
        arms |= {f"k_pmlp_fwd<{sid},{g},{a}>" for g in (0, 1) for a in (0, 1)}
    for sid in (111, 212, 222):
        arms |= {f"k_pblock_fwd<{sid},{a}>" for a in (0, 1)}
        arms |= {f"k_pmlp_bwd<{sid},{g},{a}>" for g in (0, 1) for a in (0, 1)}
    for sid in (111, 212):
        arms |= {f"k_pmlp_bwd<{sid},LIN,{a}>" for a in (0, 1)}
    arms |= {f"k_plin_fwd<{c}{c}>" for c in (1, 2, 4)} | {f"k_plin_bwd<{c}{c}>" for c in (1, 2)}
    for ci in (1, 2, 4):
        for co in (1, 2, 4):
            arms |= {f"k_plinx_fwd<{ci}{co}>", f"k_plinx_bwd<{ci}{co}>", f"k_plinx_bwd<{ci}{co},LEAN>"}
    return arms


TABLES = {"mlp_fwd": MLP_FWD_KERNEL_CASES, "block_fwd": BLOCK_FWD_KERNEL_CASES, "mlp_bwd": MLP_BWD_KERNEL_CASES,
          "block_bwd": BLOCK_BWD_KERNEL_CASES, "lin_fwd": LIN_FWD_KERNEL_CASES, "lin_bwd": LIN_BWD_KERNEL_CASES,
          "plinx_fwd": PLINX_FWD_KERNEL_CASES, "plinx_bwd": PLINX_BWD_KERNEL_CASES}


# ---- one case end to end (both tiers) ------------------------------------------------------------------------------------------
TOL_FWD, TOL_BWD = 2e-6, 3e-6      # the tighter of the bars the existing tests of the same pass hold (emulation / device files)


def run_case(kind, lib, cfg, device="cpu", stream=0, guard=False, seed=0, mark=None, expect_n_wg=None, inp=None):
    """inputs, the engine call, the float64 reference with its bounds, both assertions.  Returns (got, ratios, n_wg)."""
    cus, tiles = cu_count(device), cfg["B"] * cfg["S"] // TILE
    name = f"{kind}:{cfg.get('sid', '')}{cfg.get('c', '')}{cfg.get('ci', '')}-{cfg.get('co', '')} T={tiles}"
    n_wg = None
    if kind == "mlp_fwd":
        inp = inp or mlp_inputs(cfg, seed)
        n_wg = n_wg_for(tiles, PMLP_FWD_CAP)
        got, want, tol = run_mlp_forward(lib, cfg, inp, device, stream, guard), ref_mlp_forward(inp, cfg["act"]), TOL_FWD
    elif kind == "block_fwd":
        inp = inp or block_inputs(cfg, seed)
        n_wg = n_wg_for(tiles, PBLOCK_FWD_CAP)
        got, want, tol = run_block_forward(lib, cfg, inp, device, stream, guard), ref_block_forward(inp, cfg["act"]), TOL_FWD
    elif kind == "mlp_bwd":
        inp = inp or mlp_inputs(cfg, seed, backward=True)
        inp = inp if mark is None else mark_tile(inp, mark, cfg["S"])
        n_wg = mlp_backward_n_wg(lib, cfg)
        got = run_mlp_backward(lib, cfg, inp, device, stream, guard)
        want, tol = ref_mlp_backward(inp, cfg["act"], tiles, n_wg, cfg["xpre"]), TOL_BWD
    elif kind == "block_bwd":
        inp = inp or block_inputs(cfg, seed, backward=True)
        inp = inp if mark is None else mark_tile(inp, mark, cfg["S"], keys=("gout",))
        c, ch = cfg["chans"]
        n_wg = mlp_backward_n_wg(lib, dict(cfg, chans=(c, ch, c)))
        got = run_block_backward(lib, cfg, inp, device, stream, guard)
        xp = None if not cfg["act"] else ("grad" if cfg["act"] == ACT_DGRAD else "pre")
        want, tol = ref_mlp_backward(inp, 1 if cfg["act"] else 0, tiles, n_wg, xp, lin=True), TOL_BWD
    elif kind == "lin_fwd":
        inp = inp or linear_inputs(cfg, seed)
        n_wg = n_wg_for(tiles, plin_fwd_cap(cfg["c"], cus))
        got, want, tol = run_linear_forward(lib, cfg, inp, device, stream, guard), ref_linear(inp), TOL_FWD
    elif kind == "lin_bwd":
        inp = inp or linear_inputs(cfg, seed, backward=True)
        inp = inp if mark is None else mark_tile(inp, mark, cfg["S"])
        n_wg = linear_backward_n_wg(lib, cfg)
        got = run_linear_backward(lib, cfg, inp, device, stream, guard)
        want, tol = ref_linear(inp, tiles, n_wg), TOL_BWD
    elif kind == "plinx_fwd":
        inp = inp or plinx_inputs(cfg, seed)
        n_wg = n_wg_for(tiles, plinx_fwd_cap(cus))
        got, want, tol = run_plinx_forward(lib, cfg, inp, device, stream, guard), ref_plinx_forward(inp, cfg["flags"]), TOL_FWD
    else:
        inp = inp or plinx_inputs(cfg, seed, backward=True)
        inp = inp if mark is None else mark_tile(inp, mark, cfg["S"])
        n_wg = plinx_backward_n_wg(lib, cfg, inp, cus)
        got = run_plinx_backward(lib, cfg, inp, device, stream, guard)
        want, tol = ref_plinx_backward(inp, cfg["flags"], tiles, n_wg), TOL_BWD
    if expect_n_wg is not None:
        assert n_wg == expect_n_wg, (name, "the grid this case was designed for", expect_n_wg, "the library's", n_wg)
    return got, check(name, got, want, tol), n_wg


def cap_of(kind, cfg, cus):
    """the workgroup cap of the kernel a case of `kind` launches on a chip of `cus` compute units"""
    if kind in ("mlp_fwd", "block_fwd"):
        return PMLP_FWD_CAP if kind == "mlp_fwd" else PBLOCK_FWD_CAP
    if kind in ("mlp_bwd", "block_bwd"):
        return PMLP_BWD_CAP
    if kind == "lin_fwd":
        return plin_fwd_cap(cfg["c"], cus)
    if kind == "lin_bwd":
        return PLIN_BWD_CAP
    if kind == "plinx_fwd":
        return plinx_fwd_cap(cus)
    lean = not cfg["want_gx"] and cfg["flags"] == 0 and not cfg["gated"]
    return plinx_bwd_cap(cfg["ci"], cfg["co"], lean, cus)


def with_tiles(cfg, t):
    b, s = shape_of_tiles(t)
    return dict(cfg, B=b, S=s, T=t)


def round_tiles(which, cap):
    """tile counts around R = 4 cap tiles per round: "R-1", "R", "R+1" (the nearest T >= R + 1 that factors by 3 or 5), "2R+1\""""
    r = 4 * cap
    return {"R-1": r - 1, "R": r, "R+1": second_round_tiles(cap), "2R+1": 2 * r + 1}[which]


# ---- the activation on its tails: gelu(0 + s) through a zero weight, a unit gate and skip = s ---------------------------------
ACT_SPECIAL = (0.0, -0.0, 1e-30, -1e-30, 1e-20, -1e-20, 30.0, -30.0, 1e4, -1e4, 1e19, -1e19, 3e38, -3e38)


def activation_grid():
    """(1, 32, S) fp32: [-13, 13] in steps of 0.002, the special values, padded with 0.5 to whole tiles"""
    v = torch.cat([torch.linspace(-13.0, 13.0, 13001, dtype=torch.float64).float(), torch.tensor(ACT_SPECIAL, dtype=torch.float32)])
    n = -(-v.numel() // (32 * 32)) * 32 * 32
    return torch.cat([v, torch.full((n - v.numel(),), 0.5)]).reshape(1, 32, n // 32).contiguous()


def run_activation_routes(lib, device="cpu", stream=0):
    """sc_gelu / sc_gelu_both through sc_pointwise_linear_forward_ex(ACT), sc_pointwise_mlp_forward and
    sc_pointwise_block_forward(SC_ACT_GELU_DGRAD): dict(s, gelu = {route: tensor}, dgelu = {route: tensor}) on the host"""
    s = activation_grid()
    B, C, S = s.shape
    sd = s.to(device)
    zero, one = torch.zeros(C, C, device=device), torch.ones(C, device=device)
    x = torch.randn(B, C, S, generator=torch.Generator().manual_seed(1)).to(device)
    new = lambda: torch.full((B, C, S), NAN, device=device)
    a, b, y, pre, c = new(), new(), new(), new(), new()
    lib.pointwise_linear_forward_ex(B, C, C, S, ACT, _p(x), _p(zero), 0, _p(sd), _p(one), _p(a), 0, stream)
    lib.pointwise_mlp_forward(B, C, C, C, S, ACT_GELU, _p(x), _p(zero), 0, _p(zero), 0, _p(sd), _p(one), _p(b), stream)
    lib.pointwise_block_forward(B, C, C, S, ACT_DGRAD, _p(sd), _p(sd), _p(zero), 0, _p(zero), 0, _p(zero), 0, _p(one), _p(y), _p(pre),
                                _p(c), stream)
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()
    return dict(s=s, gelu={"k_plinx_fwd": a.cpu(), "k_pmlp_fwd": b.cpu(), "k_pblock_fwd out": c.cpu(), "k_pblock_fwd y": y.cpu()},
                dgelu={"k_pblock_fwd pre": pre.cpu()})


def check_activation(got):
    """|gelu - gelu64| <= 0.5 |v| 1.5e-7 + the counted roundings (gelu_err), the stored derivative within dgelu_err of
    Phi + v phi, every value finite, gelu(v) == v from 30 on, -0.0 or a tiny negative number below -30, and on [-8, -4] a
    relative error below what 1.5e-7 absolute on erfc allows"""
    s = got["s"]
    v = s.double()
    want, bound = gelu64(v), gelu_err(v)
    q, _, err_q, _ = erfc_parts(v)
    tail = (v >= -8) & (v <= -4)
    rel_limit = (err_q[tail] + U * q[tail]) / q[tail] + U     # h2 = q / 2 carries err_q / 2 and one rounding; v h2 one more
    worst = {}
    for name, t in got["gelu"].items():
        assert bool(torch.isfinite(t).all()), name
        err = (t.double() - want).abs()
        worst[name] = float((err / bound.clamp_min(1e-300))[bound > 0].max())
        assert bool((err <= bound).all()), (name, worst[name])
        assert bool((err[bound == 0] == 0).all()), name
        assert torch.equal(t[s >= 30], s[s >= 30]), name
        low = t[s <= -30].double()
        assert bool((low <= 0).all()) and bool((low.abs() <= 2.0 ** -126 * v[s <= -30].abs()).all()), name
        rel = (t.double()[tail] - want[tail]).abs() / want[tail].abs()
        assert bool((rel <= rel_limit).all()), (name, float((rel / rel_limit).max()))
        assert bool((t[(s < 0)] <= 0).all()) and bool((t[s > 0] >= 0).all()), name
    dwant, dbound = dgelu64(v), dgelu_err(v)
    for name, t in got["dgelu"].items():
        assert bool(torch.isfinite(t).all()), name
        err = (t.double() - dwant).abs()
        worst[name] = float((err / dbound).max())
        assert bool((err <= dbound).all()), (name, worst[name])
    print("activation: worst |err| / bound", {k: f"{r:.3f}" for k, r in worst.items()})
    return worst


# ---- the bare float64 formulas: differentiable (float64 tensors pass through, so autograd of a caller's leaves works) -------
def _dd(t):
    return None if t is None else (t if t.dtype == torch.float64 else t.detach().double().cpu())


def _flat(t):
    return t.reshape(t.shape[0], t.shape[1], -1)


def linear64(x, w, b=None):
    """W x + b over the channels of (B, C, *spatial); w: (out, in[, 1])"""
    x, w, b = _dd(x), _dd(w), _dd(b)
    out = torch.einsum("oc,bcs->bos", w.reshape(w.shape[0], w.shape[1]), _flat(x)) + _vec(None if b is None else b.reshape(-1))
    return out.reshape(x.shape[0], w.shape[0], *x.shape[2:])


def mlp64(x, w1, b1, w2, b2, skip=None, gate=None, act=0):
    """act(W2 gelu(W1 x + b1) + b2 + gate (.) skip); gate: any shape with c_out elements"""
    z = linear64(gelu64(linear64(x, w1, b1)), w2, b2)
    if skip is not None:
        z = z + _dd(gate).reshape(1, -1, *([1] * (z.dim() - 2))) * _dd(skip)
    return gelu64(z) if act else z


def plinx64(x, w, b, skip, gate, flags):
    """(out, pre-activation) of the forward pass of sc_kernels_plinx.h"""
    x = _dd(x)
    z = linear64(gelu64(x) if flags & XACT else x, w, b)
    if skip is not None:
        z = z + _dd(gate).reshape(1, -1, *([1] * (z.dim() - 2))) * _dd(skip)
    return (gelu64(z) if flags & ACT else z), z


def block64(conv, x, ws, bs, w1, b1, w2, b2, gate, act):
    """(s, y, out) of the block pass"""
    s = _dd(conv) + linear64(x, ws, bs)
    y = gelu64(s) if act else s
    return s, y, mlp64(y, w1, b1, w2, b2, x, gate, act)


def grads64(fn, tensors, gout):
    """float64 autograd: fn(*leaves) on double copies of `tensors` (None stays None), backward with gout.
    Returns (out, [gradient or None per tensor])"""
    leaves = [None if t is None else t.detach().double().cpu().requires_grad_(True) for t in tensors]
    out = fn(*leaves)
    out.backward(gout.detach().double().cpu())
    return out.detach(), [None if t is None else t.grad for t in leaves]


def assert_zero_outside_tile(got, cfg, tile):
    """gx / gskip / gin of a marked-tile case: not all zero inside the tile, exactly zero everywhere else"""
    b, px = divmod(tile, cfg["S"] // TILE)
    for k in ("gx", "gskip", "gin"):
        if got.get(k) is not None:
            rest = got[k].clone()
            assert bool((rest[b, :, TILE * px:TILE * (px + 1)] != 0).any()), k
            rest[b, :, TILE * px:TILE * (px + 1)] = 0
            assert bool((rest == 0).all()), k
