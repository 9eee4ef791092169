"""What the tests of the point-cloud discrete-continuous convolutions share: the case table of the recorder and the
tests, the seeded inputs of a case, and a float64 helper that evaluates the layer and its gradients with a dense Psi
taken from a layer's psi_idx / psi_vals (or from any list of entries).  The loader of the verbatim reference, rel_l2 and
fp32_randn are disco_reference's.  torch on the host, no engine."""
import os

import numpy as np
import torch

from disco_reference import (GOLDEN, fp32_randn, gamma, load_reference_module, reference_available, rel_l2,  # noqa: F401
                             worst_ratio)

GENERAL, MFMA = 1, 2


# ---- cases: constructor arguments of the layer, point counts, batch ----------------------------------------------------
def _case(n_in=150, n_out=70, c_in=4, c_out=6, kernel_shape=(2, 4), batch=2, transposed=False, float64=False,
          lonely=False, **kw):
    ks = kernel_shape if isinstance(kernel_shape, int) else list(kernel_shape)
    return dict(kwargs=dict(in_channels=c_in, out_channels=c_out, kernel_shape=ks, **kw), n_in=n_in, n_out=n_out,
                batch=batch, transposed=transposed, float64=float64, lonely=lonely)


# lonely: output point 3 is moved to (5, 5), far from every input point: its rows of Psi are empty, its output the bias
CASES = {
    "default": _case(lonely=True),
    "kernel_shape_3x4_r0.2": _case(kernel_shape=(3, 4), radius_cutoff=0.2),
    "kernel_shape_3": _case(kernel_shape=3),
    "groups2": _case(groups=2),
    "depthwise": _case(c_in=4, c_out=4, groups=4),
    "no_bias": _case(bias=False),
    "float64_grids": _case(float64=True),
    "transpose_default": _case(n_in=70, n_out=150, transposed=True),
    "transpose_grouped": _case(n_in=70, n_out=150, groups=2, transposed=True),
    "transpose_r0.2_3x4": _case(n_in=70, n_out=150, kernel_shape=(3, 4), radius_cutoff=0.2, transposed=True),
}
ATTRS = ("kernel_shape", "kernel_size", "groups", "groupsize", "n_in", "n_out")
NUMERIC_ATTRS = ("kernel_size", "groups", "groupsize", "n_in", "n_out")
LONELY = 3


def case_grids(cfg, seed):
    """(grid_in, grid_out, quadrature_weights) of a case: seeded uniform clouds of the unit square, weights rand / n_in
    (strictly positive)"""
    g = torch.Generator().manual_seed(seed)
    grid_in, grid_out = torch.rand(2, cfg["n_in"], generator=g), torch.rand(2, cfg["n_out"], generator=g)
    q = torch.rand(cfg["n_in"], generator=g)
    q = (q + (q == 0)) / cfg["n_in"]
    if cfg["lonely"]:
        grid_out[:, LONELY] = 5.0
    if cfg["float64"]:
        grid_in, grid_out, q = grid_in.double(), grid_out.double(), q.double()
    return grid_in, grid_out, q


def case_inputs(cfg, module, seed):
    """fp32 input, weight, bias (None without one) and cotangent for `module` built from cfg"""
    g = torch.Generator().manual_seed(seed + 1000)
    kw = cfg["kwargs"]
    x = fp32_randn((cfg["batch"], kw["in_channels"], cfg["n_in"]), g)
    w = fp32_randn(tuple(module.weight.shape), g) * float(1.0 / np.sqrt(module.groupsize))
    b = None if module.bias is None else fp32_randn((kw["out_channels"],), g)
    return x, w, b, fp32_randn((cfg["batch"], kw["out_channels"], cfg["n_out"]), g)


def reference_class(transposed):
    mod = load_reference_module()
    return mod.DiscreteContinuousConvTranspose2d if transposed else mod.DiscreteContinuousConv2d


def own_class(transposed):
    import neuraloperator_amd as na
    return na.DiscreteContinuousConvTranspose2d if transposed else na.DiscreteContinuousConv2d


def build_own(cfg, seed):
    grid_in, grid_out, q = case_grids(cfg, seed)
    return own_class(cfg["transposed"])(grid_in=grid_in, grid_out=grid_out, quadrature_weights=q, **cfg["kwargs"])


# ---- float64 helper -----------------------------------------------------------------------------------------------------
def dense_psi(psi_idx, psi_vals, kernel_size, n_out, n_in):
    """(K, n_out, n_in) float64 from the reference's matrix form (row = k n_out + o, column = i); duplicates add up"""
    idx = torch.as_tensor(psi_idx).long()
    psi = torch.zeros(kernel_size * n_out, n_in, dtype=torch.float64)
    psi.index_put_((idx[0], idx[1]), torch.as_tensor(psi_vals).double(), accumulate=True)
    return psi.reshape(kernel_size, n_out, n_in)


def sparse_disco(x, weight, bias, psi, q, groups):
    """the layer in float64: psi (K, n_out, n_in) dense -- or, for a cloud too large for that, the sparse
    (K n_out, n_in) matrix --, x (B, C, n_in), weight (C_out, C / groups, K)"""
    if psi.is_sparse:
        b, c, k = x.shape[0], x.shape[1], weight.shape[2]
        z = torch.sparse.mm(psi, (q * x).reshape(b * c, -1).t())
        z = z.t().reshape(b, c, k, -1)
    else:
        z = torch.einsum("koi,bci->bcko", psi, q * x)
    b, c, k, o = z.shape
    z = z.reshape(b, groups, c // groups, k, o)
    out = torch.einsum("bgckx,gock->bgox", z, weight.reshape(groups, -1, weight.shape[1], weight.shape[2]))
    out = out.reshape(b, -1, o)
    return out if bias is None else out + bias.reshape(1, -1, 1)


def sparse_disco_with_grads(x, weight, bias, psi, q, g, groups):
    """(out, gx, gw, gbias) in float64; without a bias gbias is the sum of g over batch and points all the same"""
    x64 = x.detach().double().cpu().requires_grad_(True)
    w64 = weight.detach().double().cpu().requires_grad_(True)
    b64 = None if bias is None else bias.detach().double().cpu().requires_grad_(True)
    g64 = g.detach().double().cpu()
    out = sparse_disco(x64, w64, b64, psi, q.detach().double().cpu(), groups)
    out.backward(g64)
    return out.detach(), x64.grad, w64.grad, g64.sum(dim=(0, 2)) if b64 is None else b64.grad


def layer_psi(m, dense=True):
    if not dense:
        return torch.sparse_coo_tensor(m.psi_idx.cpu(), m.psi_vals.cpu().double(), size=(m.kernel_size * m.n_out, m.n_in))
    return dense_psi(m.psi_idx.cpu(), m.psi_vals.cpu(), m.kernel_size, m.n_out, m.n_in)


def run_module(m, rec, device):
    """the layer with the record's weight and bias, forward + backward on the record's x and g: (out, gx, gw, gbias) as
    host numpy arrays (gbias None without a bias)"""
    with torch.no_grad():
        m.weight.copy_(torch.from_numpy(rec["weight"]))
        if m.bias is not None:
            m.bias.copy_(torch.from_numpy(rec["bias"]))
    m = m.to(device)
    m.zero_grad(set_to_none=True)
    x = torch.from_numpy(rec["x"]).to(device).requires_grad_(True)
    out = m(x)
    out.backward(torch.from_numpy(rec["g"]).to(device).to(out.dtype))
    gb = None if m.bias is None else m.bias.grad.cpu().numpy()
    return out.detach().cpu().numpy(), x.grad.cpu().numpy(), m.weight.grad.cpu().numpy(), gb


def golden_path(name):
    return os.path.join(GOLDEN, "dsparse_" + name + ".npz")


# ---- free-standing descriptors over a random Psi (the emulation and the GPU tier run the same list) ------------------
def desc_case(n_in=9, n_out=7, c_in=3, c_out=5, basis=3, batch=2, groups=1, bias=True, density=0.4, empty=(), full=(),
              route=GENERAL):
    return dict(route=route, n_in=n_in, n_out=n_out, c_in=c_in, c_out=c_out, basis=basis, batch=batch, groups=groups, bias=bias,
                density=density, empty=empty, full=full)


# empty / full: rows (o, k) of Psi without an entry / with every input point
DESC_CASES = {
    "65_columns_one_past_a_lane_chunk": desc_case(c_in=13, c_out=4, batch=5, n_in=6, n_out=5, basis=2),
    "channels_33_to_31": desc_case(c_in=33, c_out=31, batch=1, n_in=6, n_out=5, basis=2),
    "empty_rows_first_middle_last": desc_case(empty=((0, 0), (3, 1), (6, 2))),
    "a_row_with_every_input_point": desc_case(n_in=70, n_out=3, batch=1, density=0.1, full=((1, 1),)),
    "one_past_the_row_tile_33": desc_case(n_out=33, batch=1, c_in=2, c_out=2, basis=2, n_in=5),
    "rows_33_over_two_batches": desc_case(n_out=11, batch=3, c_in=2, c_out=3, basis=2, n_in=5),
    "rows_257_two_slices_of_the_weight_gradient": desc_case(n_out=257, batch=1, c_in=2, c_out=2, basis=1, n_in=4),
    "groups2": desc_case(c_in=4, c_out=6, groups=2),
    "depthwise": desc_case(c_in=4, c_out=4, groups=4),
    "depthwise_multiplier_2": desc_case(c_in=3, c_out=6, groups=3),
    "no_bias": desc_case(bias=False),
    "one_basis_function": desc_case(basis=1),
    "channels_130_past_an_lds_round": desc_case(c_in=130, c_out=3, batch=1, n_in=4, n_out=3, basis=2),
    "one_point_each_side": desc_case(n_in=1, n_out=1, batch=1, c_in=1, c_out=1, basis=1, density=1.0),
    "no_entry_at_all": desc_case(density=0.0),
    "mfma_32_32_rows_33": desc_case(c_in=32, c_out=32, n_out=33, batch=1, n_in=6, basis=2, route=MFMA),
    "mfma_64_32_rows_33_no_bias": desc_case(c_in=64, c_out=32, n_out=11, batch=3, n_in=5, basis=2, bias=False, route=MFMA),
    "mfma_32_128_rows_33": desc_case(c_in=32, c_out=128, n_out=33, batch=1, n_in=5, basis=1, route=MFMA),
    "mfma_rows_257_two_slices_129_past_a_tile": desc_case(c_in=32, c_out=32, n_out=257, batch=1, n_in=4, basis=1,
                                                          route=MFMA),
}


# Kernel-edge cases: the round, tile, slice and route edges of sc_kernels_disco_sparse.h, run on the device by
# tests/test_gpu_disco_sparse_kernels.py; EMU_KERNEL_CASES names those the one-thread-per-lane emulation finishes in
# seconds.  Groups are lettered as in that file's docstring.
def _kernel_cases():
    small = dict(n_in=6, n_out=5, basis=2, batch=1)
    c = {                                                    # a: the 128-column rounds of k_dsp_contract
        "a_forward_group_straddles_column_128": desc_case(c_in=192, c_out=6, groups=2, **small),
        "a_forward_cg130_three_rounds": desc_case(c_in=260, c_out=4, groups=2, **small),
        "a_data_gradient_c_out_130": desc_case(c_in=3, c_out=130, **small),
        "a_data_gradient_og96_straddles": desc_case(c_in=4, c_out=192, groups=2, **small),
        "a_depthwise130": desc_case(c_in=130, c_out=130, groups=130, **small),
    }
    for og in (15, 16, 17):                                  # b: the tiles of k_dsp_wgrad
        c[f"b_og{og}"] = desc_case(c_in=3, c_out=og, **small)
    for K, cg in ((3, 21), (2, 32), (5, 13)):
        c[f"b_K_cg_{K * cg}"] = desc_case(c_in=cg, c_out=5, n_in=6, n_out=5, basis=K, batch=1)
    for rows in (31, 32, 33):
        c[f"b_rows{rows}"] = desc_case(c_in=2, c_out=2, n_in=5, n_out=rows, basis=2, batch=1)
    # c: the cap of 64 slices (rows = 64 * 252 + 2 and beyond); 0 to 4 entries to a row of Psi
    c["c_slice_cap_rows_16130"] = desc_case(c_in=2, c_out=2, n_in=4, n_out=16130, basis=1, batch=1, density=0.5)
    c["c_slice_cap_mfma_rows_16400_per_slice_257"] = desc_case(c_in=32, c_out=32, n_in=4, n_out=16400, basis=1, batch=1,
                                                               density=0.5, route=MFMA)
    for i, ci in enumerate((32, 64, 128)):                   # d: matrix cores; 129 rows: one slice, a ragged last trip
        for j, co in enumerate((32, 64, 128)):
            c[f"d_mfma_{ci}_{co}_rows129"] = desc_case(c_in=ci, c_out=co, n_in=5, n_out=129, basis=(1, 3)[(i + j) % 2],
                                                       batch=1, route=MFMA)
    c["d_mfma_32_32_rows127_basis3"] = desc_case(c_in=32, c_out=32, n_in=5, n_out=127, basis=3, batch=1, route=MFMA)
    c["d_mfma_32_32_rows128_basis1"] = desc_case(c_in=32, c_out=32, n_in=5, n_out=128, basis=1, batch=1, route=MFMA)
    c["d_mfma_32_32_rows129_basis3"] = desc_case(c_in=32, c_out=32, n_in=5, n_out=43, basis=3, batch=3, route=MFMA)
    return c


KERNEL_DESC_CASES = _kernel_cases()
EMU_KERNEL_CASES = tuple(k for k in KERNEL_DESC_CASES if k[0] in "ab")
DESC_CASES.update({k: KERNEL_DESC_CASES[k] for k in EMU_KERNEL_CASES})   # the emulation tier runs DESC_CASES


def wgrad_slices(cfg):
    """(slices, per_slice) of the weight gradient as dsp_plan (sc_host_disco_sparse.h) cuts its rows"""
    rows = cfg["n_out"] * cfg["batch"]
    s = min(max(-(-rows // 256), 1), 64)
    per = -(-rows // s)
    return -(-rows // per), per


def roundings(cfg, keep=None):
    """N of (out, gx, gw, gbias): the fp32 roundings on the longest path to one element, counted in
    sc_kernels_disco_sparse.h.  An entry of Z carries z = 1 + row: the product q x (k_dsp_pack) and one fmaf per entry
    of a row of Psi (k_dsp_spmm); row = the longest row of the pattern `keep` (K, n_out, n_in), n_in without one, and
    col = its longest column over (k, o), K n_out without one.
      out    z + one fmaf per (basis function, input channel of the group) + the bias     k_dsp_contract / gemm, unpack
      gx     one fmaf per output channel of the group + one per entry of a column of Psi (col) + the
             product with q                                                              k_dsp_contract, spmm, unpack
      gw     z + one fmaf per row of a slice + the slices                                k_dsp_wgrad(_mfma), wreduce
      gbias  one addition per row of a slice (+ 1: the two halves of a wave on the matrix cores) + the slices
    Any order of summation stays below these, so they hold for both routes."""
    slices, per = wgrad_slices(cfg)
    row = cfg["n_in"] if keep is None else int(keep.sum(dim=2).max())
    col = cfg["basis"] * cfg["n_out"] if keep is None else int(keep.sum(dim=(0, 1)).max())
    z = 1 + row
    return (z + cfg["basis"] * (cfg["c_in"] // cfg["groups"]) + 1,
            cfg["c_out"] // cfg["groups"] + col + 1,
            z + per + slices,
            per + 1 + slices)


def abs_bounds(cfg, psi, keep, x, w, q, b, g):
    """((A_out, A_gx, A_gw, A_gbias), (N ..)): A is the layer and its gradients in float64 on |x|, |w|, |Psi|, |q|,
    |bias| with cotangent |g|"""
    ab = None if b is None else b.abs()
    return sparse_disco_with_grads(x.abs(), w.abs(), ab, psi.double().abs(), q.abs(), g.abs(), cfg["groups"]), roundings(cfg, keep)


def desc_psi(cfg, gen):
    """dense (K, n_out, n_in) float32 Psi of the case"""
    K, no, ni = cfg["basis"], cfg["n_out"], cfg["n_in"]
    keep = torch.rand(K, no, ni, generator=gen) < cfg["density"]
    for o, k in cfg["empty"]:
        keep[k, o] = False
    for o, k in cfg["full"]:
        keep[k, o] = True
    vals = torch.rand(K, no, ni, generator=gen) + 0.25                   # no zeros among the kept
    return torch.where(keep, vals, torch.zeros(())), keep


def desc_csr(psi, keep):
    """the two CSR forms of a dense Psi (K, n_out, n_in) with its pattern: (splits, cols, vals) int32 / int32 / fp32"""
    K, no, ni = psi.shape
    by_row = psi.permute(1, 0, 2).reshape(no * K, ni)                    # rows (o, k)
    kr = keep.permute(1, 0, 2).reshape(no * K, ni)
    out = []
    for mat, pat in ((by_row, kr), (by_row.t(), kr.t())):
        idx = torch.argwhere(pat)                                        # row-major: ascending columns within a row
        splits = torch.zeros(mat.shape[0] + 1, dtype=torch.int64)
        splits[1:] = torch.cumsum(pat.sum(dim=1), 0)
        out.append((splits.to(torch.int32), idx[:, 1].to(torch.int32).contiguous(), mat[pat].contiguous()))
    return out


def desc_inputs(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    psi, keep = desc_psi(cfg, g)
    x = fp32_randn((cfg["batch"], cfg["c_in"], cfg["n_in"]), g)
    w = fp32_randn((cfg["c_out"], cfg["c_in"] // cfg["groups"], cfg["basis"]), g) * 0.3
    q = torch.rand(cfg["n_in"], generator=g) + 0.1
    b = fp32_randn((cfg["c_out"],), g) if cfg["bias"] else None
    gout = fp32_randn((cfg["batch"], cfg["c_out"], cfg["n_out"]), g)
    return psi, keep, x, w, q, b, gout


def desc_of(cfg, nnz, **over):
    kw = dict(batch=cfg["batch"], c_in=cfg["c_in"], c_out=cfg["c_out"], n_in=cfg["n_in"], n_out=cfg["n_out"], nnz=nnz,
              basis=cfg["basis"], groups=cfg["groups"])
    kw.update(over)
    from neuraloperator_amd import _lib
    return _lib.ScEngineLib.dsparse_desc(**kw)


def csr_handle(triple):
    from neuraloperator_amd import _lib
    s, c, v = triple
    return _lib.ScEngineLib.dsparse_csr(s.data_ptr(), c.data_ptr(), v.data_ptr(), s.numel() - 1, v.numel())


def run_descriptor(lib, cfg, psi, keep, x, w, q, b, g, want=(True, True, True), device="cpu", stream=0):
    """sc_dsparse_forward + sc_dsparse_backward on tensors moved to `device`: (out, gx, gw, gbias, z)"""
    fwd, bwd = ([t.to(device) for t in m] for m in desc_csr(psi, keep))
    x, w, q, g = (t.to(device) for t in (x, w, q, g))
    b = None if b is None else b.to(device)
    d = desc_of(cfg, fwd[2].numel())
    assert lib.dsparse_path(d) == cfg["route"]
    nbytes, fbytes = lib.dsparse_workspace_bytes(d), lib.dsparse_forward_workspace_bytes(d)
    assert 0 < fbytes <= nbytes
    ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    out = torch.full(tuple(g.shape), float("nan"), device=device)
    z = torch.full((cfg["n_out"], cfg["batch"], cfg["basis"], cfg["c_in"]), float("nan"), device=device)
    lib.dsparse_forward(d, csr_handle(fwd), x.data_ptr(), q.data_ptr(), w.data_ptr(), 0 if b is None else b.data_ptr(),
                        out.data_ptr(), z.data_ptr(), ws.data_ptr(), fbytes, stream)        # its own, smaller size
    gx = torch.full_like(x, float("nan")) if want[0] else None
    gw = torch.full_like(w, float("nan")) if want[1] else None
    gb = torch.full((cfg["c_out"],), float("nan"), device=device) if want[2] else None
    ws.fill_(0xff)                                           # the backward call owes nothing to the forward call's workspace
    lib.dsparse_backward(d, csr_handle(bwd) if want[0] else None, q.data_ptr() if want[0] else 0,
                         w.data_ptr() if want[0] else 0, z.data_ptr() if want[1] else 0, g.data_ptr(),
                         *(0 if t is None else t.data_ptr() for t in (gx, gw, gb)), ws.data_ptr(), nbytes, stream)
    return tuple(None if t is None else t.cpu() for t in (out, gx, gw, gb, z))
