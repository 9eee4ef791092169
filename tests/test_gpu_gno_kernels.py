"""GPU tier: the graph neural operator kernels (sc_kernels_gno.h) at their tile, wave and scan boundaries on an MI355X,
each against a float64 formula on the host (tests/gno_reference.py): the search on lattices (pairs at distance exactly
r, coincident pairs) and at the shape edges, the transpose of a caller's CSR with columns past one wave, reduce / edge
gradient / transposed reduce and the first layer by point at every channel width the mapping distinguishes, the
default-width GNOBlock end to end, and segment_csr."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gno_reference as gr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(t):
    return t.to(DEV, copy=True)


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ 1. search
LATTICES = {1: (64, 4 / 64, 1025, 33), 2: (64, 0.25, 1025, 33), 3: (16, 3 / 16, 2049, 70)}


@pytest.fixture(scope="module")
def lattices():
    """one generator, dimensions in order: d -> (data, queries, radius)"""
    rng = np.random.default_rng(0)
    return {d: gr.lattice_points(rng, n, m, d, L) + (r,) for d, (L, r, n, m) in LATTICES.items()}


@pytest.mark.parametrize("d", [1, 2, 3])
def test_search_on_a_lattice_is_exact_and_inclusive(lattices, d):
    """no band: every query compared.  d2 <= r2 keeps the pairs at distance exactly r, and the coincident ones"""
    from neuraloperator_amd import engine
    data, queries, r = lattices[d]
    d2 = gr.squared_distances(data, queries)
    ref = gr.radius_search(data, queries, r, True)
    on_r, coincident = int((d2 == r * r).sum()), int((d2 == 0.0).sum())
    print(f"d={d}: {on_r} pairs at distance r, {coincident} coincident, degree {len(ref['neighbors_index']) / len(queries):.0f}")
    assert on_r >= 10 and coincident >= 1
    rows, cols = np.nonzero(d2 <= r * r)
    np.testing.assert_array_equal(cols, ref["neighbors_index"])              # the helper keeps the boundary pairs
    got = engine.radius_search(_dev(torch.from_numpy(data)), _dev(torch.from_numpy(queries)), r, True)
    assert got["neighbors_index"].dtype == torch.int64 and got["neighbors_row_splits"].dtype == torch.int64
    assert got["weights"].dtype == torch.float32
    np.testing.assert_array_equal(_np(got["neighbors_row_splits"]), ref["neighbors_row_splits"])
    np.testing.assert_array_equal(_np(got["neighbors_index"]), ref["neighbors_index"])
    idx = _np(got["neighbors_index"])
    assert np.all(np.diff(idx)[rows[1:] == rows[:-1]] > 0), "ascending data index within a row"
    want = d2[rows, cols].astype(np.float32)                                 # exact in float64, exactly representable
    assert np.all(want.astype(np.float64) == d2[rows, cols])
    want[want == 0] = np.float32(1e-14)
    w = _np(got["weights"])
    assert np.array_equal(w.view(np.int32), want.view(np.int32)), "weights are float32(d2) bit for bit"
    assert np.all(w[d2[rows, cols] == 0.0] == np.float32(1e-14))


def _points(seed, n, d):
    return torch.rand(n, d, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


SEARCH_SHAPES = [(1, 1), (63, 7), (64, 8), (65, 9), (1023, 31), (1024, 32), (1025, 33), (2049, 4097), (300, 8193)]


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("n,m", SEARCH_SHAPES)
def test_search_at_the_shape_edges(d, n, m):
    """chunk, tile, wave and workgroup edges; the last two shapes take the row-split scan (4096 items a pass) through
    one and two carries.  Queries inside the 1e-5 r band are excluded from the comparison, at most 1 % of them."""
    from neuraloperator_amd import engine
    r = {1: 0.004, 2: 0.05, 3: 0.12}[d]
    data, queries = _points(10 * d + n, n, d), _points(77 + d + m, m, d)
    ref = gr.radius_search(data.numpy(), queries.numpy(), r, True)
    keep = ~gr.band_queries(data.numpy(), queries.numpy(), r)
    print(f"d={d} n={n} m={m}: excluded {100 * (1 - keep.mean()):.3f} % of the queries, "
          f"degree {len(ref['neighbors_index']) / m:.1f}")
    assert 1 - keep.mean() <= 0.01
    got = engine.radius_search(_dev(data), _dev(queries), r, True)
    assert got["neighbors_index"].dtype == torch.int64 and got["neighbors_row_splits"].dtype == torch.int64
    rs, idx, w = _np(got["neighbors_row_splits"]), _np(got["neighbors_index"]), _np(got["weights"])
    assert rs.shape == (m + 1,) and rs[0] == 0 and rs[-1] == idx.size == w.size and np.all(np.diff(rs) >= 0)
    rrs, ridx = ref["neighbors_row_splits"], ref["neighbors_index"]
    np.testing.assert_array_equal(np.diff(rs)[keep], np.diff(rrs)[keep])
    row, rrow = np.repeat(np.arange(m), np.diff(rs)), np.repeat(np.arange(m), np.diff(rrs))
    if idx.size > 1:
        assert np.all(np.diff(idx)[row[1:] == row[:-1]] > 0), "ascending data index within a row"
    np.testing.assert_array_equal(idx[keep[row]], ridx[keep[rrow]])
    np.testing.assert_allclose(w[keep[row]], ref["weights"][keep[rrow]], rtol=1e-6, atol=0)


# --------------------------------------------------------------------------------------------------------- 2. transpose
def _transpose_case():
    """300 rows over 4500 columns (two passes of the column scan): columns of 0, 64, 65 and 3000 edges, and one row of
    5000 unsorted duplicates that those long columns are cut from"""
    rng = np.random.default_rng(21)
    rows, cols, long_row = 300, 4500, 117
    lengths = rng.integers(0, 9, size=rows)
    lengths[4], lengths[long_row] = 0, 5000
    splits, index = gr.random_csr(rng, rows, cols, lengths)
    special = {7: 0, 4400: 3000, 64: 64, 4097: 65}                           # column: edges
    index[np.isin(index, list(special))] = 8
    at = int(splits[long_row])
    for col, count in special.items():
        index[at:at + count] = col
        at += count
    assert at <= splits[long_row + 1]
    seg = index[splits[long_row]:splits[long_row + 1]]
    rng.shuffle(seg)                                                         # in place: the long columns interleave
    counts = np.bincount(index, minlength=cols)
    assert all(counts[col] == count for col, count in special.items()) and len(index) > 4096
    return splits, index, cols


def test_transpose_of_a_callers_csr_with_long_columns():
    from neuraloperator_amd import engine
    splits, index, cols = _transpose_case()
    want = gr.transpose_csr(splits, index, cols)
    graphs = [engine.CsrGraph(_dev(torch.from_numpy(splits)), _dev(torch.from_numpy(index)), cols) for _ in range(2)]
    first, second = graphs[0].transpose(), graphs[1].transpose()
    assert [t.dtype for t in first] == [torch.int64, torch.int32, torch.int32]
    for name, got, ref in zip(("col_splits", "perm", "row_of_edge"), first, want):
        np.testing.assert_array_equal(_np(got), ref, err_msg=name)
    assert all(torch.equal(a, b) for a, b in zip(first, second))             # the atomics' order does not show


# --------------------------------------------------------------- 3. reduce, edge gradient, transposed reduce, segment sum
CHANNELS = [1, 2, 5, 31, 32, 33, 63, 64, 65, 128, 130]
LENGTHS = [0, 1, 2, 63, 64, 65, 129, 1000, 0]


def _err(got, ref):
    return gr.rel_l2(_np(got), _np(ref))


def _reduce_combinations(splits, index, n, c, b, rng, bar=1e-5):
    """KernelIntegralFn forward and backward in every combination of the emulation tier's test_reduce_and_edge_grad,
    and SegmentCsrFn, against the float64 formula under autograd; each launched twice for the same bits"""
    from neuraloperator_amd import engine
    E = len(index)
    ts, ti = torch.from_numpy(splits), torch.from_numpy(index)
    graph = engine.CsrGraph(_dev(ts), _dev(ti), n)
    seg_graph = engine.CsrGraph(_dev(ts), None, 0, n_edges=E)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))       # noqa: E731
    w = torch.from_numpy(rng.random(E).astype(np.float32))
    worst = 0.0
    for kb in (False, True):
        K = t(*((b, E, c) if kb else (E, c)))
        for fmode in (None, "batched") if kb else (None, "unbatched", "batched"):
            Fv = None if fmode is None else t(*((b, n, c) if fmode == "batched" else (n, c)))
            for use_w in (False, True):
                for mean in (False, True):
                    tag = (c, b, kb, fmode, use_w, mean)
                    K64 = K.double().requires_grad_(True)
                    F64 = None if Fv is None else Fv.double().requires_grad_(True)
                    ref = gr.csr_reduce_torch(K64, ts, F64, ti, w.double() if use_w else None, mean)
                    g = t(*ref.shape)
                    ref.backward(g.double())
                    runs = []
                    for _ in range(2):
                        Kd = _dev(K).requires_grad_(True)
                        Fd = None if Fv is None else _dev(Fv).requires_grad_(True)
                        out = engine.KernelIntegralFn.apply(Kd, Fd, graph, _dev(w) if use_w else None, mean)
                        out.backward(_dev(g))
                        runs.append([out.detach(), Kd.grad] + ([] if Fd is None else [Fd.grad]))
                    out, gK = runs[0][:2]
                    assert out.shape == ref.shape and gK.shape == K.shape, tag
                    errs = [_err(out, ref), _err(gK, K64.grad)]
                    if Fv is not None:
                        assert runs[0][2].shape == Fv.shape, tag
                        errs.append(_err(runs[0][2], F64.grad))
                    worst = max(worst, *errs)
                    assert max(errs) <= bar, (tag, errs)
                    assert all(torch.equal(u, v) for u, v in zip(*runs)), tag        # fixed order, no float atomics
        for mean in (False, True):                                           # segment sum / mean of K itself
            K64 = K.double().requires_grad_(True)
            ref = gr.csr_reduce_torch(K64, ts, mean=mean)
            g = t(*ref.shape)
            ref.backward(g.double())
            runs = []
            for _ in range(2):
                Kd = _dev(K).requires_grad_(True)
                out = engine.SegmentCsrFn.apply(Kd, seg_graph, mean)
                out.backward(_dev(g))
                runs.append([out.detach(), Kd.grad])
            errs = [_err(runs[0][0], ref), _err(runs[0][1], K64.grad)]
            worst = max(worst, *errs)
            assert runs[0][0].shape == ref.shape and max(errs) <= bar, ("segment", c, b, kb, mean, errs)
            assert all(torch.equal(u, v) for u, v in zip(*runs))
    return worst


@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("c", CHANNELS)
def test_reduce_edge_grad_and_transposed_reduce(c, b):
    rng = np.random.default_rng(1000 * b + c)
    n = 50
    splits, index = gr.random_csr(rng, len(LENGTHS), n, np.array(LENGTHS))
    print(f"c={c} b={b}: worst rel-L2 {_reduce_combinations(splits, index, n, c, b, rng):.1e}")


def test_reduce_with_one_row_of_20000_edges():
    rng = np.random.default_rng(7)
    n = 50
    splits, index = gr.random_csr(rng, 6, n, np.array([3, 0, 20000, 65, 1, 7]))
    print(f"worst rel-L2 {_reduce_combinations(splits, index, n, 3, 2, rng):.1e}")


# ------------------------------------------------------------------------------------------- 4. first layer by point
@pytest.mark.parametrize("with_bias", [True, False])
@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("gelu", [True, False])
@pytest.mark.parametrize("c", [1, 16, 33, 64, 70, 128, 256])
def test_edge_lift_and_backward(c, gelu, batched, with_bias):
    from neuraloperator_amd import engine
    rng = np.random.default_rng(c)
    lengths = np.array([0, 1, 65, 40, 3, 200])
    rows, n, b, dy, dx, cf = len(lengths), 9, 2, 4, 3, 2
    splits, index = gr.random_csr(rng, rows, n, lengths)
    graph = engine.CsrGraph(_dev(torch.from_numpy(splits)), _dev(torch.from_numpy(index)), n)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))       # noqa: E731
    host = [t(n, dy), t(rows, dx), t(c, dy + dx + (cf if batched else 0))] + ([t(c)] if with_bias else []) \
        + ([t(b, n, cf)] if batched else [])
    leaves = [_dev(v).requires_grad_(True) for v in host]
    yy, xx, WW = leaves[:3]
    bb = leaves[3] if with_bias else None
    Py, Px = F.linear(yy, WW[:, :dy]), F.linear(xx, WW[:, dy:dy + dx])
    if batched:
        Py = Py + F.linear(leaves[-1], WW[:, dy + dx:])
    H = engine.EdgeLiftFn.apply(Py, Px, bb, graph, gelu)
    gH = t(*H.shape)
    H.backward(_dev(gH))
    # the dense formula with the concatenated first Linear, float64
    ref_leaves = [v.double().requires_grad_(True) for v in host]
    ry, rx, rW = ref_leaves[:3]
    idx = torch.from_numpy(index)
    rep = torch.repeat_interleave(torch.arange(rows), torch.from_numpy(np.diff(splits)))
    agg = torch.cat([ry[idx], rx[rep]], -1)
    if batched:
        agg = torch.cat([agg.unsqueeze(0).expand(b, -1, -1), ref_leaves[-1][:, idx]], -1)
    pre = F.linear(agg, rW, ref_leaves[3] if with_bias else None)
    Href = F.gelu(pre) if gelu else pre
    Href.backward(gH.double())
    assert H.shape == Href.shape
    assert _err(H, Href) <= 1e-5
    for i, (mine, ref) in enumerate(zip(leaves, ref_leaves)):
        assert mine.grad.shape == ref.grad.shape and _err(mine.grad, ref.grad) <= 1e-5, i


# ----------------------------------------------------------------------------------------- 5. the default-width block
# transform type -> (in_channels, channels of f_y).  "linear" and "nonlinear" multiply the kernel's out_channels by f_y
# channel by channel (integral_transform.py:193-198), so f_y carries out_channels there, and the kernel that reads f_y
# as an input ("nonlinear") takes in_channels = out_channels; "nonlinear_kernelonly" runs with in_channels = 2 proper.
BLOCK_CASES = {"linear": (2, 12), "nonlinear": (12, 12), "nonlinear_kernelonly": (2, 2)}


@pytest.mark.parametrize("transform_type", sorted(BLOCK_CASES))
def test_default_width_block_end_to_end(transform_type):
    """GNOBlock with its default [128, 256, 128] kernel MLP and 32-frequency embedding (384 -> 128 -> 256 -> 128 -> 12),
    forward and backward, against the float64 helper formula.  The bar of each quantity is max(project bar, 4 x the
    error of the SAME formula evaluated in plain fp32 torch on the host): it does not rest on the engine."""
    from neuraloperator_amd import GNOBlock
    in_ch, f_ch = BLOCK_CASES[transform_type]
    radius, batch = 0.2, 2
    g = torch.Generator().manual_seed(31)
    y, x = torch.rand(300, 3, generator=g), torch.rand(200, 3, generator=g)
    band = gr.band_queries(y.numpy(), x.numpy(), radius)
    print(f"{transform_type}: excluded {100 * band.mean():.2f} % of the queries")
    assert band.mean() <= 0.01
    x = x[torch.from_numpy(~band)]
    f = torch.randn(batch, 300, f_ch, generator=g)
    gout = torch.randn(batch, x.shape[0], 12, generator=g)
    torch.manual_seed(32)
    block = GNOBlock(in_channels=in_ch, out_channels=12, coord_dim=3, radius=radius, transform_type=transform_type,
                     use_open3d_neighbor_search=False)
    fcs = block.integral_transform.channel_mlp.fcs
    assert [fc.out_features for fc in fcs] == [128, 256, 128, 12] and block.pos_embedding.num_frequencies == 32
    assert fcs[0].in_features == 384 + (in_ch if transform_type.startswith("nonlinear") else 0)
    assert block.integral_transform.lift_route()
    params = [p.detach().clone() for fc in fcs for p in (fc.weight, fc.bias)]
    block = block.to(DEV)
    fd = _dev(f).requires_grad_(True)
    out = block(_dev(y), _dev(x), fd)
    out.backward(_dev(gout))
    got = [out, fd.grad] + [p.grad for fc in block.integral_transform.channel_mlp.fcs for p in (fc.weight, fc.bias)]
    nbrs = {k: torch.from_numpy(v) for k, v in gr.radius_search(y.numpy(), x.numpy(), radius).items()}
    assert nbrs["neighbors_index"].numel() > 0

    def helper(dtype):
        ps = [p.clone().to(dtype).requires_grad_(True) for p in params]
        fv = f.clone().to(dtype).requires_grad_(True)
        h = gr.integral_transform(gr.sinusoidal_embedding(y.to(dtype), 32), gr.sinusoidal_embedding(x.to(dtype), 32),
                                  nbrs, ps[0::2], ps[1::2], f_y=fv, transform_type=transform_type)
        h.backward(gout.to(dtype))
        return [h.detach(), fv.grad] + [p.grad for p in ps]

    ref, plain = helper(torch.float64), helper(torch.float32)
    names = ["out", "grad:f_y"] + [f"grad:fcs.{i}.{k}" for i in range(4) for k in ("weight", "bias")]
    failed = []
    for name, mine, r64, r32 in zip(names, got, ref, plain):
        assert mine.shape == r64.shape, name
        err, own = _err(mine, r64), _err(r32, r64)
        bar = max(2e-5 if name.startswith("grad:fcs") else 1e-5, 4 * own)
        print(f"{transform_type} {name}: engine {err:.2e}, fp32 restatement {own:.2e}, bar {bar:.2e}")
        if not err <= bar:
            failed.append((name, err, bar))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------- 6. segment_csr
@pytest.mark.parametrize("c", [3, 70])
def test_segment_csr(c):
    from neuraloperator_amd.gno import segment_csr
    rng = np.random.default_rng(60 + c)
    b = 2
    lengths = np.array(LENGTHS)
    splits = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    E, ts = int(splits[-1]), torch.from_numpy(splits)
    for batched in (False, True):
        src = torch.from_numpy(rng.standard_normal((b, E, c) if batched else (E, c)).astype(np.float32))
        for indptr in (ts, ts.unsqueeze(0).repeat(b, 1)):
            for reduction in ("sum", "mean"):
                tag = (c, batched, indptr.dim(), reduction)
                sd = _dev(src).requires_grad_(True)
                out = segment_csr(sd, _dev(indptr), reduction)
                want = gr.csr_reduce(src.numpy(), splits, mean=reduction == "mean")
                assert out.shape == want.shape and gr.rel_l2(_np(out), want) <= 1e-5, tag
                g = torch.from_numpy(rng.standard_normal(want.shape).astype(np.float32))
                out.backward(_dev(g))
                s64 = src.double().requires_grad_(True)
                gr.csr_reduce_torch(s64, ts, mean=reduction == "mean").backward(g.double())
                assert sd.grad.shape == src.shape and _err(sd.grad, s64.grad) <= 1e-5, tag
    with pytest.raises(ValueError):
        segment_csr(_dev(src), _dev(ts), "max")
