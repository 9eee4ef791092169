"""Helper of the point-cloud finite-difference tests: the float64 closed form of the reference's
``get_non_uniform_fd_weights`` / ``non_uniform_fd`` (neuralop/losses/differentiation.py:728-855) in plain numpy on the
CPU, the case tables, the exclusion mask and the bounds.

The reference's ``lstsq`` returns, per point, the minimum-norm solution of the (d + 1) x k system ``A w = e``: row 0 of
``A`` is ones, row i + 1 the coordinate differences, masked columns zeroed.  That is ``w = A^T (A A^T)^-1 e``; its
regularised form ``(A^T A + lam I) w = A^T e`` is ``w = A^T (A A^T + lam I)^-1 e`` (push-through identity).  The recorder
(tests/record_nufd.py) checks this against the verbatim function where the reference exists.

Exclusion mask (from the points in float64 alone, never from the code under test): a point is left out of a comparison
where the answer is not determined to the bar --
  * its k-th and (k + 1)-th sorted distances differ by less than 1e-5 relative (which neighbour is the last one),
  * with a radius, a distance beyond the first three lies within 1e-5 relative of the radius (kept or masked),
  * with a radius, the 3rd and 4th distances are that close while the 4th lies outside the radius (which one is "always
    kept"),
  * the singular values of its masked A, coordinate rows scaled by the k-th distance, have a ratio above 1e3.
At most 1 % of a recorded fixture's points may be excluded; the recorder asserts it."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
TILE, QPW, QPB, CAP = 1024, 8, 32, 128          # NUFD_TILE, NUFD_QPW, NUFD_QPB, NUFD_CAP of sc_kernels_nufd.h
LANES = 64                                      # data points a wave takes at a time (the chunk loop of k_knn)
LAMBDA = 1e-6
BAND, MAX_COND, MAX_EXCLUDED = 1e-5, 1e3, 0.01


def gamma(n):
    return n * U / (1.0 - n * U)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nb = np.linalg.norm(b.ravel())
    return float(np.linalg.norm((a - b).ravel()) / nb) if nb > 0 else float(np.abs(a).max() if a.size else 0.0)


# ---- the closed form ----------------------------------------------------------------------------------------------------
def sorted_neighbours(points, queries=None, count=None):
    """(index, d2) of every query's data points in ascending (d2, index), the first ``count``: exact float64 distances
    of fp32-representable coordinates, a stable sort"""
    p = np.asarray(points, np.float64)
    q = p if queries is None else np.asarray(queries, np.float64)
    d2 = ((q[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    order = np.argsort(d2, axis=1, kind="stable")
    count = p.shape[0] if count is None else count
    order = order[:, :count]
    return order, np.take_along_axis(d2, order, axis=1)


def keep_mask(d2k, radius):
    """the reference's radius mask on the k sorted distances: within the radius, the first three always"""
    keep = np.ones(d2k.shape, bool)
    if radius is not None:
        keep = np.sqrt(d2k) <= radius
        keep[:, :3] = True
    return keep


def system(points, idx, keep):
    """A (N, d + 1, k) of the reference, masked columns zeroed"""
    p = np.asarray(points, np.float64)
    A = np.ones((p.shape[0], p.shape[1] + 1, idx.shape[1]))
    A[:, 1:, :] = np.transpose(p[idx] - p[:, None, :], (0, 2, 1))
    return A * keep[:, None, :]


def weights(points, idx, keep, deriv, lam=0.0):
    """w (N, n_deriv, k) = A^T (A A^T + lam I)^-1 e_{deriv + 1}; a singular system gives NaN rows (excluded points)"""
    A = system(points, idx, keep)
    n, r, k = A.shape
    G = A @ np.transpose(A, (0, 2, 1)) + lam * np.eye(r)
    E = np.zeros((r, len(deriv)))
    for j, i in enumerate(deriv):
        E[i + 1, j] = 1.0
    Y = np.full((n, r, len(deriv)), np.nan)
    for p in range(n):
        try:
            Y[p] = np.linalg.solve(G[p], E)
        except np.linalg.LinAlgError:
            pass
    return np.transpose(np.transpose(A, (0, 2, 1)) @ Y, (0, 2, 1))


def closed_form(points, k, deriv, radius=None, lam=0.0):
    """(idx (N, k), d2 (N, k), keep (N, k), w (N, n_deriv, k)) in float64"""
    idx, d2 = sorted_neighbours(points, count=k)
    keep = keep_mask(d2, radius)
    return idx, d2, keep, weights(points, idx, keep, deriv, lam)


def apply(w, idx, values):
    """values (B, N) -> (n_deriv, B, N)"""
    v = np.asarray(values, np.float64)
    return np.einsum("njm,bnm->jbn", np.asarray(w, np.float64), v[:, idx])


def adjoint(w, idx, g):
    """g (n_deriv, B, N) -> grad of the values (B, N)"""
    g = np.asarray(g, np.float64)
    contrib = np.einsum("njm,jbn->bnm", np.asarray(w, np.float64), g)
    out = np.zeros((g.shape[1], idx.shape[0]))
    for b in range(g.shape[1]):
        np.add.at(out[b], idx.ravel(), contrib[b].ravel())
    return out


def model_error(w64, idx, values, keep_points):
    """err:model -- what rounding the float64 weights to fp32 costs: fp32(w) times the fp32 values, summed in float64,
    against the float64 derivative, rel-L2 over the included points"""
    ref = apply(w64, idx, values)[..., keep_points]
    got = apply(np.asarray(w64, np.float32).astype(np.float64), idx, values)[..., keep_points]
    return rel_l2(got, ref)


# ---- exclusion ------------------------------------------------------------------------------------------------------------
def excluded(points, k, radius=None):
    """bool (N): the points left out of the comparisons (module docstring)"""
    p = np.asarray(points, np.float64)
    n = p.shape[0]
    idx, d2 = sorted_neighbours(p, count=min(k + 1, n))
    dist = np.sqrt(d2)
    out = np.zeros(n, bool)
    if n > k:
        out |= dist[:, k] - dist[:, k - 1] < BAND * dist[:, k]
    dk, ik = dist[:, :k], idx[:, :k]
    if radius is not None:
        out |= (np.abs(dk[:, 3:] - radius) < BAND * radius).any(1)
        if k > 3:
            out |= (dk[:, 3] - dk[:, 2] < BAND * dk[:, 3]) & (dk[:, 3] > radius)
    keep = keep_mask(d2[:, :k], radius)
    A = system(p, ik, keep)
    scale = np.where(dk[:, k - 1] > 0, dk[:, k - 1], 1.0)
    A[:, 1:, :] /= scale[:, None, None]
    s = np.linalg.svd(A, compute_uv=False)
    out |= ~(s[:, 0] <= MAX_COND * s[:, -1])
    return out


# ---- bounds -----------------------------------------------------------------------------------------------------------
def abs_bound(w64, idx, values, k):
    """(A, N): |derivative error| <= gamma_N A per element, A = sum_m |w_m| |v_m| in float64 and N the fp32 roundings on
    the way, counted in sc_kernels_nufd.h: the weight's own rounding to fp32 in k_nufd_weights (1; the float64 solve
    before it stays below one more, counted as 1) and one fmaf per neighbour in k_nufd_apply (k)"""
    return apply(np.abs(w64), idx, np.abs(np.asarray(values, np.float64))), k + 2


def match_by_index(idx_got, w_got, idx_ref):
    """w_got (N, J, k) reordered so that its neighbour axis follows idx_ref: rows whose index SETS agree only"""
    a, b = np.argsort(idx_got, axis=1, kind="stable"), np.argsort(idx_ref, axis=1, kind="stable")
    inv = np.empty_like(b)
    np.put_along_axis(inv, b, np.arange(idx_ref.shape[1])[None, :].repeat(idx_ref.shape[0], 0), axis=1)
    pos = np.take_along_axis(a, inv, axis=1)                 # position in got of the neighbour at each ref position
    return np.take_along_axis(np.asarray(w_got), pos[:, None, :].repeat(w_got.shape[1], 1), axis=2)


def same_sets(idx_got, idx_ref):
    return (np.sort(idx_got, axis=1) == np.sort(idx_ref, axis=1)).all(1)


def order_ok(idx, d2):
    """non-decreasing d2, ascending index among equal d2"""
    d2, di = np.asarray(d2), np.diff(np.asarray(idx), axis=1)
    a, b = d2[:, :-1], d2[:, 1:]                             # compared, not subtracted: +inf next to +inf is a tie
    return bool(np.all((b > a) | ((b == a) & (di > 0))))


# ---- recorded fixtures -------------------------------------------------------------------------------------------------
def _case(n, d, k, deriv, radius=None, reg=False, seed=0):
    return dict(n=n, d=d, k=k, deriv=list(deriv), radius=radius, reg=reg, seed=seed)


CASES = {
    "n300_d1_k3": _case(300, 1, 3, [0]),
    "n300_d2_k3": _case(300, 2, 3, [1]),
    "n300_d2_k5": _case(300, 2, 5, [0, 1]),
    "n300_d2_k9": _case(300, 2, 9, [1], seed=1),
    "n300_d2_k9_r012": _case(300, 2, 9, [0, 1], radius=0.12),
    "n300_d2_k9_reg": _case(300, 2, 9, [0, 1], reg=True, seed=2),
    "n300_d2_k32": _case(300, 2, 32, [0, 1]),
    "n513_d2_k16_r01": _case(513, 2, 16, [0], radius=0.1, seed=1),
    "n300_d3_k4": _case(300, 3, 4, [0]),
    "n257_d3_k12": _case(257, 3, 12, [2, 0, 1]),
    "n257_d3_k12_reg": _case(257, 3, 12, [2, 0, 1], reg=True, seed=1),
    "n1000_d3_k16": _case(1000, 3, 16, [2, 0, 1], seed=2),
}


def fixture_path(name):
    return os.path.join(GOLDEN, "nufd_" + name + ".npz")


def case_inputs(cfg):
    """(points (N, d), values (N,), g (n_deriv, N)) fp32 of a recorded case"""
    import torch
    gen = torch.Generator().manual_seed(cfg["seed"])
    points = torch.rand(cfg["n"], cfg["d"], generator=gen, dtype=torch.float32)
    values = torch.sin(3.0 * points.double()).sum(1).float()
    g = torch.randn(len(cfg["deriv"]), cfg["n"], generator=gen, dtype=torch.float32)
    return points.numpy(), values.numpy(), g.numpy()


# ---- free-standing descriptors (the emulation and the GPU tier run the same lists) ------------------------------------
def knn_case(n, m, d, k, kind="rand", seed=None, emu=True):
    """kind: rand; descending (every point improves the k best); nan_tenth (a tenth of the data points have a NaN
    coordinate); few_finite (fewer than k finite data points); nan_query (one query has a NaN coordinate).  emu=False
    keeps a case out of the emulation tier."""
    return dict(n=n, m=m, d=d, k=k, kind=kind, seed=seed, emu=emu)


# m = 37: a second workgroup with one wave of 5 queries and three empty waves; 70: a partly filled third workgroup
KNN_CASES = {
    "whole_cloud_4": knn_case(4, 4, 3, 4),
    "whole_cloud_32": knn_case(32, 32, 2, 32),
    "one_below_a_tile": knn_case(TILE - 1, 37, 1, 3),
    "one_tile": knn_case(TILE, 37, 2, 5),
    "one_past_a_tile": knn_case(TILE + 1, 37, 3, 12),
    "one_past_two_tiles": knn_case(2 * TILE + 1, 70, 2, 31),
    "one_chunk_of_lanes": knn_case(64, 9, 3, 16),
    "every_point_improves": knn_case(3 * TILE - 40, 5, 1, 9, kind="descending"),
    "every_point_improves_k32": knn_case(2 * TILE + 3, 3, 1, 32, kind="descending"),
    # the buffer of a query is ranked at the second and third chunk of 64 lanes, with k = 32 kept each time
    "every_point_improves_n129_k32": knn_case(2 * LANES + 1, 3, 1, 32, kind="descending"),
    # k = 32 is the largest the engine takes (NUFD_KMAX; sc_knn refuses 33): the whole cloud but one point
    "all_but_one_point_n33_k32": knn_case(33, 33, 2, 32),
    "nan_in_a_tenth_of_the_data": knn_case(300, 37, 3, 12, kind="nan_tenth"),
    "fewer_than_k_finite_points": knn_case(200, 9, 2, 9, kind="few_finite"),
    "a_query_with_a_nan": knn_case(100, 9, 2, 5, kind="nan_query"),
}
# query counts on the queries-per-wave (8) and per-workgroup (32) edges, the last workgroup partly filled
for _m in (1, QPW - 1, QPW, QPW + 1, QPB - 1, QPB, QPB + 1, 2 * QPB + 1):
    KNN_CASES[f"queries_m{_m}"] = knn_case(200, _m, 2, 5)
# data counts on the 64-lane chunk: the first (cnt > 64) and the second compaction of a query's buffer
for _n in (LANES - 1, LANES, LANES + 1, 2 * LANES - 1, 2 * LANES, 2 * LANES + 1):
    for _k in (32, 3):
        for _d in (1, 3):
            KNN_CASES[f"lanes_n{_n}_k{_k}_d{_d}"] = knn_case(_n, 9, _d, _k)
MAX_TIE_SHARE = 0.05


def knn_expected(cfg, data, queries):
    """(index (m, c), d2 (m, c), tie (m), exact (m)) of the float64 sort on (d2 with NaN -> +inf, index), c = min(k + 1,
    n) columns.  tie: the k-th and (k + 1)-th distances are FINITE and within BAND (relative): which is the last
    neighbour is not determined.  exact: every gap between consecutive finite distances of the c columns exceeds BAND, so
    the fp32 rounding of d2 (a few 2^-24 relative) cannot reorder them: the whole index row is determined.  +inf entries
    are ordered by index alone and are always determined."""
    k, n = cfg["k"], cfg["n"]
    p, q = np.asarray(data, np.float64), np.asarray(queries, np.float64)
    d2 = ((q[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    d2[np.isnan(d2)] = np.inf
    order = np.argsort(d2, axis=1, kind="stable")[:, :min(k + 1, n)]
    d2 = np.take_along_axis(d2, order, axis=1)
    dist = np.sqrt(d2)
    with np.errstate(invalid="ignore"):
        close = (dist[:, 1:] - dist[:, :-1] < BAND * dist[:, 1:]) & np.isfinite(dist[:, 1:])
    tie = close[:, k - 1] if n > k else np.zeros(len(q), bool)
    return order, d2, tie, ~close.any(1)


def knn_tie_share(cfg):
    data, queries = knn_inputs(cfg)
    return float(knn_expected(cfg, data, queries)[2].mean())


def knn_inputs(cfg):
    """(data (n, d), queries (m, d)) fp32"""
    rng = np.random.default_rng(1000 * cfg["n"] + 10 * cfg["k"] + cfg["d"] if cfg.get("seed") is None else cfg["seed"])
    n, m, d = cfg["n"], cfg["m"], cfg["d"]
    if cfg["kind"] in ("nan_tenth", "few_finite", "nan_query"):          # queries of their own: none is a NaN data point
        data, queries = rng.random((n, d), dtype=np.float32), rng.random((m, d), dtype=np.float32)
        if cfg["kind"] == "nan_tenth":
            bad = np.arange(3, n, 10)
            data[bad, bad % d] = np.nan
        elif cfg["kind"] == "few_finite":                    # k - 4 finite points, most of them behind the first ranking
            finite = np.array([3, 70, 130, 150, n - 1, 5, 90, 111])[:cfg["k"] - 4]
            keep = data[finite].copy()
            data[:, 0] = np.nan
            data[finite] = keep
        else:
            queries[4, 1] = np.nan
        return data, queries
    if cfg["kind"] == "descending":
        # 1-d points stored in descending distance from the last ones, which are the queries: every data point beats
        # the current k-th best, so the buffer fills and is ranked at every other chunk
        data = ((n - np.arange(n)) / np.float32(n)).astype(np.float32).reshape(n, 1)
        return data, data[n - m:].copy()
    data = rng.random((n, d), dtype=np.float32)
    queries = data[rng.permutation(n)[:m]].copy() if m <= n else rng.random((m, d), dtype=np.float32)
    return data, queries


def stencil_case(n, d, k, deriv, radius=None, reg=False, batch=1, kind="rand"):
    return dict(n=n, d=d, k=k, deriv=list(deriv), radius=radius, reg=reg, batch=batch, kind=kind)


STENCIL_CASES = {
    "d1_k3": stencil_case(70, 1, 3, [0]),
    "d2_k3": stencil_case(90, 2, 3, [1, 0]),
    "d3_k4": stencil_case(90, 3, 4, [2], batch=3),
    "d2_k5_batch3": stencil_case(300, 2, 5, [0, 1], batch=3),
    "d2_k9_radius": stencil_case(130, 2, 9, [0, 1], radius=0.17),
    "d2_k9_radius_down_to_three": stencil_case(130, 2, 9, [0], radius=0.06, kind="three"),
    "d3_k12_reg": stencil_case(257, 3, 12, [0, 1, 2], reg=True),
    "d3_k16_eight_derivatives": stencil_case(140, 3, 16, [2, 0, 1, 1, 0, 2, 2, 0], batch=3),
    "d2_k31": stencil_case(70, 2, 31, [1]),
    "whole_cloud_32": stencil_case(32, 2, 32, [0, 1]),
    "whole_cloud_4": stencil_case(4, 3, 4, [0, 1, 2]),
    "two_identical_points": stencil_case(60, 2, 9, [0, 1], kind="duplicate"),
}


def stencil_inputs(cfg):
    """(points (N, d), values (B, N), g (n_deriv, B, N)) fp32"""
    rng = np.random.default_rng(100 * cfg["n"] + 10 * cfg["k"] + cfg["d"])
    n, d = cfg["n"], cfg["d"]
    points = rng.random((n, d), dtype=np.float32)
    if cfg["kind"] == "duplicate":
        points[41] = points[7]
    phase = rng.random((cfg["batch"], 1, d))
    values = np.sin(3.0 * points.astype(np.float64)[None] + phase).sum(-1).astype(np.float32)
    g = rng.standard_normal((len(cfg["deriv"]), cfg["batch"], n)).astype(np.float32)
    return points, values, g


def lattice_points(side=5):
    """side x side lattice with spacing 1 / 4 (exact in fp32): every distance ties with others"""
    ax = np.arange(side, dtype=np.float32) / 4
    return np.stack(np.meshgrid(ax, ax, indexing="ij"), -1).reshape(-1, 2)


def line_points(n=40):
    """n points of the line y = x / 2 in 2-d, coordinates exact in fp32: every stencil is collinear"""
    t = (np.random.default_rng(3).permutation(4 * n)[:n].astype(np.float32)) / 64
    return np.stack([t, t / 2], -1)


# ---- the bars, shared by the CPU and the GPU tier -------------------------------------------------------------------
def helper_results(points, values, g, k, deriv, radius=None, reg=False):
    """what the closed form gives for (points, values (B, N), g (n_deriv, B, N)): dict(indices, weights, derivatives,
    grad, excluded, model); g is zeroed at the excluded points first (in place)"""
    ex = excluded(points, k, radius)
    g[..., ex] = 0.0
    idx, _, _, w = closed_form(points, k, deriv, radius, LAMBDA if reg else 0.0)
    w = np.where(ex[:, None, None], 0.0, w)                  # an excluded point's stencil meets a zero cotangent only
    return dict(indices=idx, weights=w, derivatives=apply(w, idx, values), grad=adjoint(w, idx, g), excluded=ex,
                model=model_error(w, idx, values, ~ex))


def fixture_results(name):
    """the same dict from a recorded fixture, and its inputs (points, values (1, N), g (n_deriv, 1, N))"""
    rec = dict(np.load(fixture_path(name)))
    cfg = CASES[name]
    ex = excluded(rec["points"], cfg["k"], cfg["radius"])
    assert np.all(rec["g"][:, ex] == 0.0)
    ref = dict(indices=rec["ref:indices"].astype(np.int64), weights=rec["ref:weights"],
               derivatives=rec["ref:derivatives"][:, None], grad=rec["ref:grad:values"][None], excluded=ex,
               model=float(rec["err:model"]))
    return ref, (rec["points"], rec["values"][None], rec["g"][:, None])


def check(label, ref, values, k, got_idx, got_d2, got_w, got_der, got_grad):
    """the bars of the issue on the included points; every measured figure is printed before it is asserted"""
    inc = ~ref["excluded"]
    n = got_idx.shape[0]
    got_idx, got_w = np.asarray(got_idx), np.asarray(got_w, np.float64)
    # neighbour sets, order, range
    assert got_idx.min() >= 0 and got_idx.max() < n
    assert order_ok(got_idx, got_d2), label
    assert same_sets(got_idx[inc], ref["indices"][inc]).all(), label
    # weights by neighbour index
    wm = match_by_index(got_idx[inc], got_w[inc], ref["indices"][inc])
    e_w = rel_l2(wm, ref["weights"][inc])
    rowsum = np.abs(got_w[inc].sum(-1))
    rowbar = k * 2.0 ** -23 * np.abs(got_w[inc]).max(-1)
    # derivatives: per element and for the tensor
    A, nround = abs_bound(ref["weights"], ref["indices"], values, k)
    err = np.abs(np.asarray(got_der, np.float64) - ref["derivatives"])[..., inc]
    worst = float((err / np.maximum(gamma(nround) * A[..., inc], 1e-300)).max())
    e_d = rel_l2(np.asarray(got_der)[..., inc], ref["derivatives"][..., inc])
    bar_d = max(1e-5, 2.0 * ref["model"])
    e_g = rel_l2(got_grad, ref["grad"])
    print(f"{label}: excluded {int((~inc).sum())} of {n}, weights {e_w:.2e}, row sums {float((rowsum / np.maximum(rowbar, 1e-300)).max()):.2f} "
          f"of their bound, derivatives {e_d:.2e} (bar {bar_d:.1e}, model {ref['model']:.1e}), worst element {worst:.3f} "
          f"of its bound, grad {e_g:.2e}")
    assert e_w <= 1e-5, label
    assert np.all(rowsum <= rowbar), label
    assert worst <= 1.0, label
    assert e_d <= bar_d, label
    assert e_g <= 1e-5, label
