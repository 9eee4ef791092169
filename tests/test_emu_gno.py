"""CPU tier: the graph neural operator kernels (sc_kernels_gno.h) in host emulation against the float64 helper
(tests/gno_reference.py): radius search, CSR transpose, fused reduce, edge gradient, first layer by point, refusals."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gno_reference as gr
from emu_engine import engine_on_emulation
from neuraloperator_amd import _lib, engine


@pytest.fixture(scope="module")
def emu():
    with engine_on_emulation() as lib:
        yield lib


def _points(seed, n, d):
    return torch.rand(n, d, generator=torch.Generator().manual_seed(seed), dtype=torch.float32)


def _check_search(data, queries, radius, return_norm=True):
    got = engine.radius_search(data, queries, radius, return_norm)
    ref = gr.radius_search(data.numpy(), queries.numpy(), radius, True)
    keep = ~gr.band_queries(data.numpy(), queries.numpy(), radius) if len(data) and len(queries) else np.ones(len(queries), bool)
    assert keep.mean() > 0.9
    rs, idx = got["neighbors_row_splits"].numpy(), got["neighbors_index"].numpy()
    assert got["neighbors_row_splits"].dtype == torch.int64 and got["neighbors_index"].dtype == torch.int64
    assert rs[0] == 0 and rs[-1] == len(idx) and np.all(np.diff(rs) >= 0)
    rrs, ridx = ref["neighbors_row_splits"], ref["neighbors_index"]
    for q in range(len(queries)):
        mine = idx[rs[q]:rs[q + 1]]
        assert np.all(np.diff(mine) > 0), "ascending data index"
        if keep[q]:
            np.testing.assert_array_equal(mine, ridx[rrs[q]:rrs[q + 1]])
            if return_norm:
                np.testing.assert_allclose(got["weights"].numpy()[rs[q]:rs[q + 1]], ref["weights"][rrs[q]:rrs[q + 1]],
                                           rtol=1e-6, atol=0)
    return got


# a full tile plus a ragged one with a ragged last workgroup; fewer queries than one wave carries; exactly one tile
SEARCH_SHAPES = [(gr.GNO_TILE + 37, gr.GNO_QPB + 5), (50, 5), (gr.GNO_TILE, gr.GNO_QPB)]


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("n,m", SEARCH_SHAPES)
def test_radius_search(emu, d, n, m):
    data, queries = _points(10 * d + n, n, d), _points(77 + d + m, m, d)
    queries[0] = data[3]                                     # a coincident pair: kept, weight 1e-14
    got = _check_search(data, queries, {1: 0.02, 2: 0.1, 3: 0.2}[d])
    rs = got["neighbors_row_splits"].numpy()
    first = got["neighbors_index"].numpy()[rs[0]:rs[1]]
    assert 3 in first
    assert got["weights"].numpy()[rs[0]:rs[1]][list(first).index(3)] == np.float32(1e-14)


def test_radius_takes_every_point_and_none(emu):
    data, queries = _points(1, 70, 3), _points(2, 9, 3)
    got = _check_search(data, queries, 10.0)
    assert got["neighbors_index"].numel() == 70 * 9
    got = engine.radius_search(data, queries, 1e-9, True)
    assert got["neighbors_index"].numel() == 0 and got["weights"].numel() == 0
    assert got["neighbors_row_splits"].tolist() == [0] * 10
    for n, m in ((0, 4), (5, 0)):                            # valid empty inputs: no launch, zero-filled splits
        got = engine.radius_search(_points(1, n, 2), _points(2, m, 2), 0.5)
        assert got["neighbors_index"].numel() == 0 and got["neighbors_row_splits"].tolist() == [0] * (m + 1)
    assert "weights" not in got


def test_csr_transpose_of_any_csr(emu):
    rng = np.random.default_rng(5)
    rows, cols = 37, 23
    lengths = rng.integers(0, 9, size=rows)
    lengths[4], lengths[9] = 0, 150                          # an empty row; a row with many duplicates, unsorted
    splits, index = gr.random_csr(rng, rows, cols, lengths)
    index[index == 7] = 8                                    # an empty column
    g = engine.CsrGraph(torch.from_numpy(splits), torch.from_numpy(index), cols)
    col_splits, perm, row = (t.numpy() for t in g.transpose())
    rcs, rperm, rrow = gr.transpose_csr(splits, index, cols)
    np.testing.assert_array_equal(col_splits, rcs)
    np.testing.assert_array_equal(row, rrow)
    assert sorted(perm.tolist()) == list(range(len(index)))  # a permutation
    for j in range(cols):
        sl = perm[col_splits[j]:col_splits[j + 1]]
        assert np.all(np.diff(sl) > 0) and np.all(index[sl] == j)
    np.testing.assert_array_equal(perm, rperm)
    assert g.transpose()[1] is g.transpose()[1]              # built once, kept


def test_csr_transpose_across_the_scan_carry(emu):
    """4100 columns: the column scan takes two passes (256 x 16 items each) and carries the first pass's total"""
    rng = np.random.default_rng(6)
    rows, cols = 40, 4100
    splits, index = gr.random_csr(rng, rows, cols, rng.integers(0, 9, size=rows))
    index[:70] = 4098                                        # a column past the carry, longer than one wave
    index[70:80] = 4095
    g = engine.CsrGraph(torch.from_numpy(splits), torch.from_numpy(index), cols)
    for got, ref in zip(g.transpose(), gr.transpose_csr(splits, index, cols)):
        np.testing.assert_array_equal(got.numpy(), ref)


def _csr_with_bad_indices(rng, lengths, cols):
    """a caller's CSR whose index holds -1, cols and a large value among valid entries: (splits, index, valid mask)"""
    splits, index = gr.random_csr(rng, len(lengths), cols, np.array(lengths))
    bad = rng.permutation(len(index))[:12]
    index[bad[:4]], index[bad[4:8]], index[bad[8:]] = -1, cols, 1 << 40
    valid = (index >= 0) & (index < cols)
    assert valid.sum() == len(index) - 12
    return splits, index, valid


def test_out_of_range_indices_join_nothing(emu):
    rng = np.random.default_rng(9)
    cols, c, b = 11, 5, 2
    splits, index, valid = _csr_with_bad_indices(rng, [0, 3, 70, 9, 1, 30], cols)
    E, rows = len(index), len(splits) - 1
    graph = engine.CsrGraph(torch.from_numpy(splits), torch.from_numpy(index), cols)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))       # noqa: E731
    # reduce with F: such an edge contributes 0 (the mean still divides by the row's length)
    K, Fv, w = t(b, E, c), t(b, cols, c), torch.from_numpy(rng.random(E).astype(np.float32))
    Kz, safe = K.numpy() * valid[None, :, None], np.where(valid, index, 0)
    for mean in (False, True):
        out = engine._csr_reduce(graph, K, Fv, w, mean)
        assert gr.rel_l2(out.numpy(), gr.csr_reduce(Kz, splits, Fv.numpy(), safe, w.numpy(), mean)) < 1e-6
    g = t(b, rows, c)
    gK = engine._csr_edge_grad(graph, g, Fv, w, False, True)
    assert float(gK[:, torch.from_numpy(~valid)].abs().sum()) == 0.0 and float(gK.abs().sum()) > 0.0
    # transpose: such an edge joins no column
    col_splits, perm, row = (v.numpy() for v in graph.transpose())
    ids = np.nonzero(valid)[0]
    rcs, rperm, _ = gr.transpose_csr(splits, index[valid], cols)
    np.testing.assert_array_equal(col_splits, rcs)
    assert col_splits[-1] == valid.sum()
    np.testing.assert_array_equal(perm[:len(ids)], ids[rperm])
    assert np.all(perm[len(ids):] == -1)
    np.testing.assert_array_equal(row, np.repeat(np.arange(rows), np.diff(splits)))
    gF = engine._csr_reduce(graph, K, g, w, False, transposed=True)             # walks perm: the -1 tail is never read
    v = Kz * g.numpy()[:, np.repeat(np.arange(rows), np.diff(splits))] * w.numpy()[None, :, None]
    want = np.zeros((b, cols, c))
    np.add.at(want, (slice(None), safe), v)
    assert gr.rel_l2(gF.numpy(), want) < 1e-6
    # first layer by point: H = 0 on such an edge, and no gradient through it
    for gelu in (True, False):
        Py, Px, bias = (v.requires_grad_(True) for v in (t(b, cols, c), t(rows, c), t(c)))
        H = engine.EdgeLiftFn.apply(Py, Px, bias, graph, gelu)
        assert float(H.detach()[:, torch.from_numpy(~valid)].abs().sum()) == 0.0
        rep = np.repeat(np.arange(rows), np.diff(splits))
        leaves = [v.detach().double().requires_grad_(True) for v in (Py, Px, bias)]
        pre = leaves[0][:, safe] + leaves[1][rep] + leaves[2]
        Href = (F.gelu(pre) if gelu else pre) * torch.from_numpy(valid)[None, :, None]
        assert gr.rel_l2(H.detach().numpy(), Href.detach().numpy()) < 1e-6
        gH = t(*H.shape)
        H.backward(gH)
        Href.backward(gH.double())
        for mine, ref in zip((Py, Px, bias), leaves):
            assert gr.rel_l2(mine.grad.numpy(), ref.grad.numpy()) < 1e-5


LENGTHS = [0, 1, 65, 300, 7, 0, 2]                           # empty, single, past one wave, many passes of every group


@pytest.mark.parametrize("c", [1, 3, 32, 33, 64, 70, 128])
def test_reduce_and_edge_grad(emu, c):
    rng = np.random.default_rng(c)
    rows, n, b = len(LENGTHS), 11, 2
    splits, index = gr.random_csr(rng, rows, n, np.array(LENGTHS))
    E = len(index)
    graph = engine.CsrGraph(torch.from_numpy(splits), torch.from_numpy(index), n)
    w = torch.from_numpy(rng.random(E).astype(np.float32))
    for kb in (False, True):
        K = torch.from_numpy(rng.standard_normal((b, E, c) if kb else (E, c)).astype(np.float32))
        for fmode in (None, "batched") if kb else (None, "unbatched", "batched"):
            Fv = None if fmode is None else torch.from_numpy(
                rng.standard_normal((b, n, c) if fmode == "batched" else (n, c)).astype(np.float32))
            for use_w in (False, True):
                for mean in (False, True):
                    ww = w if use_w else None
                    out = engine._csr_reduce(graph, K, Fv, ww, mean)
                    ref = gr.csr_reduce(K.numpy(), splits, None if Fv is None else Fv.numpy(), index,
                                        None if ww is None else ww.numpy(), mean)
                    if Fv is not None and Fv.dim() == 3 and not kb:
                        ref = np.stack([gr.csr_reduce(K.numpy(), splits, Fv[i].numpy(), index,
                                                      None if ww is None else ww.numpy(), mean) for i in range(b)])
                    assert out.shape == ref.shape
                    assert gr.rel_l2(out.numpy(), ref) < 1e-6, (kb, fmode, use_w, mean)
                    assert torch.equal(out, engine._csr_reduce(graph, K, Fv, ww, mean))       # fixed order
                    # <reduce(K), g> = <K, edge_grad(g)>
                    g = torch.from_numpy(rng.standard_normal(out.shape).astype(np.float32))
                    gK = engine._csr_edge_grad(graph, g, Fv, ww, mean, kb)
                    assert gK.shape == K.shape
                    lhs = float((out.double() * g.double()).sum())
                    rhs = float((K.double() * gK.double()).sum())
                    scale = float(out.double().norm() * g.double().norm()) + 1e-30
                    assert abs(lhs - rhs) <= 1e-5 * scale, (kb, fmode, use_w, mean, lhs, rhs)
                    if Fv is not None:                       # the transposed reduce is the adjoint in F
                        gF = engine._csr_reduce(graph, K, g, ww, mean, transposed=True)
                        if gF.dim() == 3 and Fv.dim() == 2:
                            gF = gF.sum(0)
                        rhs = float((Fv.double() * gF.double()).sum())
                        assert abs(lhs - rhs) <= 1e-5 * scale, ("gF", kb, fmode, use_w, mean, lhs, rhs)


@pytest.mark.parametrize("c,batched,gelu", [(3, False, True), (33, True, True), (70, True, False), (32, False, False)])
def test_edge_lift_and_backward(emu, c, batched, gelu):
    rng = np.random.default_rng(c)
    lengths = np.array([0, 1, 65, 40, 3])
    rows, n, b, dy, dx, cf = len(lengths), 9, 2, 4, 3, 2
    splits, index = gr.random_csr(rng, rows, n, lengths)
    graph = engine.CsrGraph(torch.from_numpy(splits), torch.from_numpy(index), n)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))       # noqa: E731
    y, x, W, bias = t(n, dy), t(rows, dx), t(c, dy + dx + (cf if batched else 0)), t(c)
    f = t(b, n, cf) if batched else None
    leaves = [v.clone().requires_grad_(True) for v in (y, x, W, bias)] + ([f.clone().requires_grad_(True)] if batched else [])
    yy, xx, WW, bb = leaves[:4]
    Py, Px = F.linear(yy, WW[:, :dy]), F.linear(xx, WW[:, dy:dy + dx])
    if batched:
        Py = Py + F.linear(leaves[4], WW[:, dy + dx:])
    H = engine.EdgeLiftFn.apply(Py, Px, bb, graph, gelu)
    gH = t(*H.shape)
    H.backward(gH)
    # the dense formula with the concatenated first Linear, float64
    ref_leaves = [v.detach().double().requires_grad_(True) for v in leaves]
    ry, rx, rW, rb = ref_leaves[:4]
    idx = torch.from_numpy(index)
    rep = torch.repeat_interleave(torch.arange(rows), torch.from_numpy(np.diff(splits)))
    agg = torch.cat([ry[idx], rx[rep]], -1)
    if batched:
        agg = torch.cat([agg.unsqueeze(0).expand(b, -1, -1), ref_leaves[4][:, idx]], -1)
    pre = F.linear(agg, rW, rb)
    Href = F.gelu(pre) if gelu else pre
    Href.backward(gH.double())
    assert H.shape == Href.shape
    assert gr.rel_l2(H.detach().numpy(), Href.detach().numpy()) < 1e-5
    for mine, ref in zip(leaves, ref_leaves):
        assert gr.rel_l2(mine.grad.numpy(), ref.grad.numpy()) < 1e-5


def test_refusals_before_any_launch(emu):
    L = emu.lib
    buf = torch.zeros(64, dtype=torch.int64)
    p = buf.data_ptr()
    R = _lib.ScEngineLib.radius_desc
    for desc, args in [(R(0, 4, 4, 0.5), (p, p, p, p)), (R(4, 4, 4, 0.5), (p, p, p, p)), (R(2, -1, 4, 0.5), (p, p, p, p)),
                       (R(2, 4, -1, 0.5), (p, p, p, p)), (R(2, 4, 4, 0.5), (None, p, p, p)),
                       (R(2, 4, 4, 0.5), (p, None, p, p)), (R(2, 4, 4, 0.5), (p, p, None, p)),
                       (R(2, 4, 4, 0.5), (p, p, p, None)), (R(2, 4, 4, -1.0), (p, p, p, p))]:
        assert L.sc_radius_count(ctypes.byref(desc), *args, None) != 0
        assert "sc_engine" in emu.lib.sc_last_error().decode()
    assert L.sc_radius_count(None, p, p, p, p, None) != 0
    assert L.sc_radius_fill(ctypes.byref(R(5, 4, 4, 0.5)), p, p, p, 3, p, p, None) != 0
    assert L.sc_radius_fill(ctypes.byref(R(2, 4, 4, 0.5)), p, p, p, -3, p, p, None) != 0
    assert L.sc_radius_fill(ctypes.byref(R(2, 4, 4, 0.5)), p, p, p, 3, None, p, None) != 0
    assert L.sc_radius_fill(ctypes.byref(R(2, 4, 4, 0.5, True)), p, p, p, 3, p, None, None) != 0
    C = _lib.ScEngineLib.csr_desc
    for desc in (C(-1, 4, 4), C(4, -1, 4), C(4, 4, -1), C(4, 4, 4, n_splits=4)):
        assert L.sc_csr_transpose(ctypes.byref(desc), p, p, p, p, p, p, 1 << 20, None) != 0
        assert L.sc_csr_transpose_workspace_bytes(ctypes.byref(desc)) == 0
    ok = C(4, 4, 4)
    assert L.sc_csr_transpose(ctypes.byref(ok), None, p, p, p, p, p, 1 << 20, None) != 0
    assert L.sc_csr_transpose(ctypes.byref(ok), p, p, p, p, p, p, 4, None) != 0          # workspace too small
    D = _lib.ScEngineLib.csr_reduce_desc
    good = dict(rows=4, n_edges=4, channels=3, splits=p)
    for bad in (dict(rows=-1), dict(n_edges=-1), dict(channels=0), dict(batch=0), dict(splits=0), dict(n_splits=4),
                dict(k_batch_stride=-1), dict(n_f=-1)):
        desc = D(**{**good, **bad})
        assert L.sc_csr_reduce(ctypes.byref(desc), p, None, p, None) != 0
        assert L.sc_csr_edge_grad(ctypes.byref(desc), p, None, p, None) != 0
    assert L.sc_csr_reduce(ctypes.byref(D(**good)), None, None, p, None) != 0
    assert L.sc_csr_reduce(ctypes.byref(D(**good)), p, None, None, None) != 0
    assert L.sc_csr_edge_grad(ctypes.byref(D(**good)), None, None, p, None) != 0
    assert L.sc_csr_edge_grad(ctypes.byref(D(**good, perm=p)), p, None, p, None) != 0
    E = _lib.ScEngineLib.edge_lift_desc
    good = dict(rows=4, n_edges=4, n_py=4, channels=3, splits=p, index=p)
    for bad in (dict(rows=-1), dict(n_edges=-1), dict(n_py=-1), dict(channels=0), dict(batch=0), dict(splits=0),
                dict(index=0), dict(n_splits=6), dict(act=7)):
        desc = E(**{**good, **bad})
        assert L.sc_edge_lift(ctypes.byref(desc), p, p, p, p, None) != 0
        assert L.sc_edge_lift_bwd(ctypes.byref(desc), p, p, p, p, p, None) != 0
    assert L.sc_edge_lift(ctypes.byref(E(**good)), None, p, p, p, None) != 0
    assert L.sc_edge_lift_bwd(ctypes.byref(E(**good)), p, p, p, None, p, None) != 0
    # valid empty problems are not refusals
    assert L.sc_csr_reduce(ctypes.byref(D(rows=0, n_edges=0, channels=3, splits=p)), None, None, None, None) == 0
    assert L.sc_csr_transpose(ctypes.byref(C(0, 3, 0)), None, None, p, None, None, None, 0, None) == 0
    out = torch.ones(2, 4, 3)
    assert L.sc_csr_reduce(ctypes.byref(D(rows=4, n_edges=0, channels=3, batch=2, splits=p)), None, None,
                           out.data_ptr(), None) == 0
    assert float(out.abs().sum()) == 0.0                     # the owed zero fill
