"""CPU tier: the point-cloud discrete-continuous convolution kernels (sc_kernels_disco_sparse.h) in host emulation through
the C-ABI against the float64 helper (tests/disco_sparse_reference.py): free-standing descriptors over a random Psi with
duplicate-free rows -- forward, data, weight and bias gradient, the route, every refusal before any launch, a CSR with
out-of-range columns between guard bands, bit-identical repeats.  The emulation runs one OS thread per lane: tiny extents."""
import ctypes

import pytest
import torch

import disco_sparse_reference as ds
from emu_engine import engine_on_emulation
from neuraloperator_amd import _lib


@pytest.fixture(scope="module")
def emu():
    with engine_on_emulation() as lib:
        yield lib


CASES, _cfg, _inputs, _csr = ds.DESC_CASES, ds.desc_case, ds.desc_inputs, ds.desc_csr
_desc, _handle = ds.desc_of, ds.csr_handle


def _run(lib, cfg, *tensors, want=(True, True, True)):
    return ds.run_descriptor(lib, cfg, *tensors, want=want)


def _want(cfg, psi, x, w, q, b, g):
    return ds.sparse_disco_with_grads(x, w, b, psi.double(), q, g, cfg["groups"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_float64_helper(emu, name):
    cfg = CASES[name]
    psi, keep, x, w, q, b, g = _inputs(cfg, 91)
    got = _run(emu, cfg, psi, keep, x, w, q, b, g)
    want = _want(cfg, psi, x, w, q, b, g)
    errs = [ds.rel_l2(a.numpy(), t.numpy()) if float(t.abs().max()) > 0 else float(a.abs().max())
            for a, t in zip(got[:4], want)]
    print(name, " ".join(f"{e:.1e}" for e in errs))
    assert max(errs) <= 1e-5, errs
    bounds, ns = ds.abs_bounds(cfg, psi, keep, x, w, q, b, g)            # per element: |got - want| <= gamma_N A
    ratios = [ds.worst_ratio(a.numpy(), t.numpy(), A.numpy(), n) for a, t, A, n in zip(got[:4], want, bounds, ns)]
    print(name, "worst |err| / (gamma_N A)", " ".join(f"{r:.3f}" for r in ratios))
    assert max(ratios) <= 1.0, ratios
    z = torch.einsum("koi,bci->obkc", psi.double(), (q * x).double())    # the saved tensor in the engine's layout
    assert float(z.abs().max()) == 0 or ds.rel_l2(got[4].numpy(), z.numpy()) <= 1e-5
    for o, k in cfg["empty"]:                                            # an empty row writes zeros
        assert float(got[4][o, :, k].abs().max()) == 0.0
    if cfg["density"] == 0.0 and b is not None:                          # no neighbour anywhere: the bias alone
        assert torch.equal(got[0], b.reshape(1, -1, 1).expand_as(got[0]))


@pytest.mark.parametrize("name", ["groups2", "65_columns_one_past_a_lane_chunk", "mfma_64_32_rows_33_no_bias"])
def test_repeats_are_bit_identical_and_one_gradient_alone_is_the_same(emu, name):
    cfg = CASES[name]
    args = _inputs(cfg, 92)
    a, c = _run(emu, cfg, *args), _run(emu, cfg, *args)
    assert all(torch.equal(u, v) for u, v in zip(a, c))
    for i in range(3):                                                   # null gx / gw / gbias in turn
        want = tuple(j == i for j in range(3))
        one = _run(emu, cfg, *args, want=want)
        assert torch.equal(one[1 + i], a[1 + i]) and sum(t is not None for t in one[1:4]) == 1
        two = _run(emu, cfg, *args, want=tuple(not v for v in want))
        assert two[1 + i] is None and all(torch.equal(two[1 + j], a[1 + j]) for j in range(3) if j != i)


def test_route_of_a_descriptor(emu):
    D = _lib.ScEngineLib.dsparse_desc
    base = dict(batch=2, n_in=100, n_out=50, nnz=1000, basis=5)
    for ci in (32, 64, 128):
        for co in (32, 64, 128):
            assert emu.dsparse_path(D(c_in=ci, c_out=co, **base)) == ds.MFMA == _lib.SC_DSPARSE_PATH_MFMA
    for ci, co, groups in ((3, 5, 1), (32, 32, 2), (64, 64, 64), (33, 32, 1), (32, 96, 1), (256, 32, 1), (4, 4, 4)):
        assert emu.dsparse_path(D(c_in=ci, c_out=co, groups=groups, **base)) == ds.GENERAL == _lib.SC_DSPARSE_PATH_GENERAL


def test_refusals_before_any_launch(emu):
    L, D = emu.lib, _lib.ScEngineLib.dsparse_desc
    cfg = _cfg(c_in=4, c_out=4)
    psi, keep, x, w, q, b, g = _inputs(cfg, 5)
    fwd, bwd = _csr(psi, keep)
    nnz = fwd[2].numel()
    buf = torch.zeros(1 << 16)
    p, n = buf.data_ptr(), buf.numel() * 4
    good = dict(batch=2, c_in=4, c_out=4, n_in=9, n_out=7, nnz=nnz, basis=3)
    hf, hb = _handle(fwd), _handle(bwd)
    bad = [dict(groups=3), dict(c_in=6, groups=3), dict(c_out=6, groups=4), dict(groups=0), dict(batch=0), dict(c_in=0),
           dict(c_out=0), dict(basis=0), dict(n_in=0), dict(n_out=0), dict(nnz=-1),
           dict(n_out=1 << 30), dict(n_in=1 << 31), dict(nnz=1 << 31),            # beyond 32-bit indices
           dict(batch=1 << 20), dict(c_in=1 << 22, c_out=1 << 22)]
    for change in bad:
        d = D(**{**good, **change})
        assert L.sc_dsparse_path(ctypes.byref(d)) == 0, change
        assert L.sc_dsparse_workspace_bytes(ctypes.byref(d)) == 0 == L.sc_dsparse_forward_workspace_bytes(ctypes.byref(d))
        assert L.sc_dsparse_forward(ctypes.byref(d), ctypes.byref(hf), p, p, p, p, p, p, p, n, None) != 0, change
        assert "sc_engine" in L.sc_last_error().decode()
        assert L.sc_dsparse_backward(ctypes.byref(d), ctypes.byref(hb), p, p, p, p, p, p, p, p, n, None) != 0, change
    ok = ctypes.byref(D(**good))
    C = _lib.ScEngineLib.dsparse_csr
    # a CSR that does not fit the descriptor: a wrong splits length, an entry count that is not desc.nnz, null arrays
    wrong_f = [C(p, p, p, 7 * 3 + 1, nnz), C(p, p, p, 7 * 3 - 1, nnz), C(p, p, p, 9, nnz), C(p, p, p, 7 * 3, nnz + 1),
               C(p, p, p, 7 * 3, nnz - 1), C(0, p, p, 7 * 3, nnz), C(p, 0, p, 7 * 3, nnz), C(p, p, 0, 7 * 3, nnz)]
    for h in wrong_f:
        assert L.sc_dsparse_forward(ok, ctypes.byref(h), p, p, p, p, p, p, p, n, None) != 0
        assert "sc_engine" in L.sc_last_error().decode()
    wrong_b = [C(p, p, p, 10, nnz), C(p, p, p, 8, nnz), C(p, p, p, 7 * 3, nnz), C(p, p, p, 9, nnz + 1),
               C(0, p, p, 9, nnz), C(p, 0, p, 9, nnz)]
    for h in wrong_b:
        assert L.sc_dsparse_backward(ok, ctypes.byref(h), p, p, p, p, p, p, p, p, n, None) != 0
    assert L.sc_dsparse_path(None) == 0 and L.sc_dsparse_workspace_bytes(None) == 0
    assert L.sc_dsparse_forward(None, ctypes.byref(hf), p, p, p, p, p, p, p, n, None) != 0
    assert L.sc_dsparse_forward(ok, None, p, p, p, p, p, p, p, n, None) != 0
    #             x  q  w  bias out z  ws
    for args in ((None, p, p, p, p, p, p), (p, None, p, p, p, p, p), (p, p, None, p, p, p, p), (p, p, p, p, None, p, p),
                 (p, p, p, p, p, None, p), (p, p, p, p, p, p, None)):
        assert L.sc_dsparse_forward(ok, ctypes.byref(hf), *args, n, None) != 0, args
    assert L.sc_dsparse_forward(ok, ctypes.byref(hf), p, p, p, p, p, p, p, 8, None) != 0     # workspace too small
    hbr = ctypes.byref(hb)
    #                    q  w  z  gout gx gw gb ws
    for csr, args in ((hbr, (p, p, p, None, p, p, p, p)), (hbr, (p, p, p, p, None, None, None, p)),
                      (hbr, (p, p, p, p, p, p, p, None)), (hbr, (None, p, p, p, p, None, None, p)),
                      (hbr, (p, None, p, p, p, None, None, p)), (hbr, (p, p, None, p, None, p, None, p)),
                      (None, (p, p, p, p, p, None, None, p))):
        assert L.sc_dsparse_backward(ok, csr, *args, n, None) != 0, args
    assert L.sc_dsparse_backward(ok, hbr, p, p, p, p, p, p, p, p, 8, None) != 0
    assert float(buf.abs().sum()) == 0.0                                 # no refused call wrote anything


def test_out_of_range_columns_leave_memory_outside_the_outputs_untouched(emu):
    """host buffers between guard bands, both CSR forms with columns below zero and beyond their range and splits beyond
    nnz: such entries count as zero, and nothing outside out, z, gx, gw, gbias and the workspace is written"""
    cfg = _cfg(c_in=4, c_out=6, groups=2)
    psi, keep, x, w, q, b, g = _inputs(cfg, 17)
    fwd, bwd = _csr(psi, keep)
    nnz = fwd[2].numel()
    spoil = torch.arange(nnz) % 5 == 2                                   # entries whose column is broken
    bad_f = (fwd[0].clone(), torch.where(spoil, torch.where(torch.arange(nnz) % 2 == 0, -1, cfg["n_in"]).int(), fwd[1]),
             fwd[2])
    bad_b = (bwd[0].clone(), torch.where(spoil, torch.where(torch.arange(nnz) % 2 == 0, -7, cfg["n_out"] * cfg["basis"]
                                                            ).int(), bwd[1]), bwd[2])
    bad_f[0][-1] = nnz + 1000                                            # splits beyond the arrays are cut to nnz
    bad_b[0][-1] = nnz + 1000
    GUARD, MARK = 4096, 1234.5
    d = _desc(cfg, nnz)
    nws = emu.dsparse_workspace_bytes(d) // 4
    sizes = dict(out=g.numel(), z=cfg["n_out"] * cfg["batch"] * cfg["basis"] * cfg["c_in"], gx=x.numel(), gw=w.numel(),
                 gb=cfg["c_out"], ws=nws)
    arena = torch.full((sum(sizes.values()) + GUARD * (len(sizes) + 1),), MARK)
    view, at, inside = {}, GUARD, torch.zeros(arena.numel(), dtype=torch.bool)
    for k, n in sizes.items():
        view[k] = arena[at:at + n]
        inside[at:at + n] = True
        at += n + GUARD
    emu.dsparse_forward(d, _handle(bad_f), x.data_ptr(), q.data_ptr(), w.data_ptr(), b.data_ptr(), view["out"].data_ptr(),
                        view["z"].data_ptr(), view["ws"].data_ptr(), nws * 4)
    emu.dsparse_backward(d, _handle(bad_b), q.data_ptr(), w.data_ptr(), view["z"].data_ptr(), g.data_ptr(),
                         view["gx"].data_ptr(), view["gw"].data_ptr(), view["gb"].data_ptr(), view["ws"].data_ptr(),
                         nws * 4)
    assert bool((arena[~inside] == MARK).all())
    # and what was computed is the layer of the Psi without the broken entries
    def without(triple, by_input):
        s, c, v = triple
        rows = torch.repeat_interleave(torch.arange(s.numel() - 1), (s[1:] - s[:-1]).long())
        ok = ~spoil
        ok_rows, ok_cols = (c[ok].long(), rows[ok]) if by_input else (rows[ok], c[ok].long())
        dense = torch.zeros(cfg["basis"], cfg["n_out"], cfg["n_in"], dtype=torch.float64)
        dense[ok_rows % cfg["basis"], ok_rows // cfg["basis"], ok_cols] = v[ok].double()
        return dense
    out, _, gw, gb = ds.sparse_disco_with_grads(x, w, b, without(fwd, False), q, g, cfg["groups"])
    _, gx, _, _ = ds.sparse_disco_with_grads(x, w, b, without(bwd, True), q, g, cfg["groups"])
    for k, t in (("out", out), ("gx", gx), ("gw", gw), ("gb", gb)):
        assert ds.rel_l2(view[k].reshape(t.shape).numpy(), t.numpy()) <= 1e-5, k
