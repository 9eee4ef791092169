"""The descriptor runs that tests/test_emu_nufd.py (host emulation, CPU tensors) and tests/test_gpu_nufd.py (MI355X)
share: each takes the device the tensors live on and checks the engine's C-ABI calls against tests/nufd_reference.py."""
import numpy as np
import torch

import nufd_reference as nr
from neuraloperator_amd import engine


def _np(t):
    return t.detach().cpu().numpy()


KNN_SENTINEL = 0x7FC0BEEF      # a NaN no kernel produces, compared as bits


def knn_through_the_c_abi(cfg, data, queries):
    """lib.knn on index and d2 buffers with m k sentinels (int64 -7, NaN) in front and behind: (index, d2) on the host,
    the guards asserted intact"""
    from neuraloperator_amd import _lib
    lib, dev, mk = _lib.get_lib(), data.device, cfg["m"] * cfg["k"]
    bi = torch.full((3 * mk,), -7, dtype=torch.int64, device=dev)
    bd = torch.full((3 * mk,), KNN_SENTINEL, dtype=torch.int32, device=dev)
    lib.knn(lib.knn_desc(cfg["d"], cfg["n"], cfg["m"], cfg["k"]), data.data_ptr(), queries.data_ptr(),
            bi[mk:].data_ptr(), bd[mk:].data_ptr(), stream=engine._stream())
    if dev.type == "cuda":
        torch.cuda.synchronize()
    for buf, sent in ((bi, -7), (bd, KNN_SENTINEL)):
        assert bool((buf[:mk] == sent).all()) and bool((buf[2 * mk:] == sent).all()), "a store outside index / d2"
    shape = (cfg["m"], cfg["k"])
    return _np(bi[mk:2 * mk].reshape(shape)), _np(bd[mk:2 * mk].view(torch.float32).reshape(shape))


def run_knn(name, dev):
    """sc_knn of m queries against n data points: sets and order against the float64 sort on (d2 with NaN -> +inf,
    index); +inf entries and rows without a near tie exactly; the same bits through the C-ABI on guarded buffers"""
    cfg = nr.KNN_CASES[name]
    data, queries = nr.knn_inputs(cfg)
    k = cfg["k"]
    td, tq = torch.from_numpy(data).to(dev), torch.from_numpy(queries).to(dev)
    idx, d2 = engine.knn_search(td, tq, k)
    assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and idx.shape == d2.shape == (cfg["m"], k)
    idx, d2 = _np(idx), _np(d2)
    ridx, rd2, tie, exact = nr.knn_expected(cfg, data, queries)
    ridx, rd2 = ridx[:, :k], rd2[:, :k]
    print(f"{name}: {int(tie.sum())} of {cfg['m']} queries with a tie at the k-th neighbour, {int(exact.sum())} rows exact")
    assert tie.mean() <= 0.05
    assert not np.isnan(d2).any() and idx.min() >= 0 and idx.max() < cfg["n"] and nr.order_ok(idx, d2)
    assert nr.same_sets(idx[~tie], ridx[~tie]).all()
    np.testing.assert_allclose(d2[~tie], rd2[~tie], rtol=1e-6, atol=0)        # both ascending
    inf = np.isinf(rd2)                                      # NaN distances: +inf in ascending index, nothing to a band
    assert np.array_equal(np.isinf(d2), inf) and np.array_equal(idx[inf], ridx[inf])
    assert np.array_equal(idx[exact], ridx[exact])           # no near tie in the row: its order is determined
    if cfg["kind"] == "few_finite":
        assert inf[:, k - 4:].all() and not inf[:, :k - 4].any()
    if cfg["kind"] == "nan_query":
        assert np.array_equal(idx[4], np.arange(k)) and np.isinf(d2[4]).all() and not np.isinf(d2[[0, 8]]).any()
    if cfg["kind"] == "nan_tenth":
        assert not inf.any() and not np.isin(idx, np.arange(3, cfg["n"], 10)).any()
    again = engine.knn_search(td, tq, k)
    assert np.array_equal(_np(again[0]), idx) and np.array_equal(_np(again[1]).view(np.int32), d2.view(np.int32))
    cidx, cd2 = knn_through_the_c_abi(cfg, td, tq)
    assert np.array_equal(cidx, idx) and np.array_equal(cd2.view(np.int32), d2.view(np.int32))


def build_and_step(points, values, g, cfg, dev):
    """stencil, derivatives and the gradient of the values on ``dev``: (stencil, derivatives, grad)"""
    st = engine.NufdStencil(torch.from_numpy(points).to(dev), cfg["k"], cfg["deriv"], cfg["radius"], cfg["reg"])
    v = torch.from_numpy(values).to(dev).requires_grad_()
    out = engine.NufdApplyFn.apply(v, st)
    out.backward(torch.from_numpy(g).to(dev))
    return st, out.detach(), v.grad


def run_stencil(name, dev):
    """knn + weights + apply + adjoint of one STENCIL_CASES entry at the issue's bars"""
    cfg = nr.STENCIL_CASES[name]
    points, values, g = nr.stencil_inputs(cfg)
    ref = nr.helper_results(points, values, g, cfg["k"], cfg["deriv"], cfg["radius"], cfg["reg"])
    assert ref["excluded"].sum() <= max(1, cfg["n"] // 50), name
    st, der, grad = build_and_step(points, values, g, cfg, dev)
    assert st.fd_weights.shape == (cfg["n"], len(cfg["deriv"]), cfg["k"]) and st.fd_weights.dtype == torch.float32
    assert der.shape == (len(cfg["deriv"]), cfg["batch"], cfg["n"]) and st.flag.dtype == torch.int32
    idx, d2 = _np(st.indices), _np(st.d2)
    nr.check(name, ref, values, cfg["k"], idx, d2, _np(st.fd_weights), _np(der), _np(grad))
    assert not np.any(_np(st.flag).astype(bool) & ~ref["excluded"])           # only an excluded point may be ill-posed
    alone = d2[:, 1] > 0
    assert np.array_equal(idx[alone, 0], np.arange(cfg["n"])[alone])
    if cfg["kind"] == "duplicate":                           # the tie at distance 0 goes by index, both stay well-posed
        assert list(idx[7, :2]) == [7, 41] and list(idx[41, :2]) == [7, 41] and not alone[7] and not alone[41]
        assert np.abs(_np(st.fd_weights)[[7, 41]]).max() > 0
    if cfg["kind"] == "three":                               # some compared points are left with exactly three neighbours
        kept = nr.keep_mask(nr.sorted_neighbours(points, count=cfg["k"])[1], cfg["radius"]).sum(1)
        assert ((kept == 3) & ~ref["excluded"]).sum() >= 3
        assert np.all(_np(st.fd_weights)[kept == 3][:, :, 3:] == 0.0)
    st2, der2, grad2 = build_and_step(points, values, g, cfg, dev)         # fixed order: the same bits
    for a, b in ((st.indices, st2.indices), (st.fd_weights, st2.fd_weights), (der, der2), (grad, grad2)):
        assert torch.equal(a, b)


def run_lattice(dev):
    """exact ties everywhere: only the order property and the derivative of a LINEAR field, exact for any tie choice"""
    points = nr.lattice_points(5)
    st = engine.NufdStencil(torch.from_numpy(points).to(dev), 5, [0, 1])
    idx, d2, w = _np(st.indices), _np(st.d2), _np(st.fd_weights).astype(np.float64)
    assert nr.order_ok(idx, d2) and int(st.flag.sum()) == 0
    assert np.array_equal(d2.astype(np.float64), ((points[idx] - points[:, None]).astype(np.float64) ** 2).sum(-1))
    values = (0.5 + 2.0 * points[:, 0] - 3.0 * points[:, 1]).astype(np.float32)[None]
    der = _np(engine.NufdApplyFn.apply(torch.from_numpy(values).to(dev), st)).astype(np.float64)
    bound = nr.gamma(5 + 2) * nr.apply(np.abs(w), idx, np.abs(values))
    print("lattice: worst error of the linear field", float(np.abs(der[0] - 2.0).max()), float(np.abs(der[1] + 3.0).max()))
    assert np.all(np.abs(der[0] - 2.0) <= bound[0]) and np.all(np.abs(der[1] + 3.0) <= bound[1])


def run_line(dev):
    """every stencil collinear: all points flagged, all weights zero, no NaN or inf anywhere"""
    points = nr.line_points(40)
    st = engine.NufdStencil(torch.from_numpy(points).to(dev), 5, [0, 1])
    assert _np(st.flag).tolist() == [1] * 40
    assert float(st.fd_weights.abs().sum()) == 0.0
    v = torch.from_numpy(points[:, 0].copy()[None]).to(dev).requires_grad_()
    out = engine.NufdApplyFn.apply(v, st)
    out.backward(torch.ones_like(out))
    for t in (st.d2, st.fd_weights, out, v.grad):
        assert bool(torch.isfinite(t).all())
    assert float(out.detach().abs().sum()) == 0.0 and float(v.grad.abs().sum()) == 0.0
    return st
