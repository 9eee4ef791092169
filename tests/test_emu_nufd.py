"""CPU tier: the point-cloud finite-difference kernels (sc_kernels_nufd.h) in host emulation against the float64 helper
(tests/nufd_reference.py): the k-nearest-neighbour search at its tile, wave and buffer edges, the weights, the apply and
its adjoint at the issue's bars, ties, collinear clouds, refusals.  tests/test_gpu_nufd.py runs the same lists on the
device."""
import ctypes

import pytest
import torch

import nufd_cases as nc
import nufd_reference as nr
from emu_engine import engine_on_emulation
from neuraloperator_amd import _lib

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def emu():
    with engine_on_emulation() as lib:
        yield lib


@pytest.mark.parametrize("name", sorted(n for n, c in nr.KNN_CASES.items() if c["emu"]))
def test_knn(emu, name):
    nc.run_knn(name, CPU)


@pytest.mark.parametrize("name", sorted(nr.STENCIL_CASES))
def test_stencil(emu, name):
    nc.run_stencil(name, CPU)


def test_lattice_of_exact_ties(emu):
    nc.run_lattice(CPU)


def test_collinear_cloud_is_flagged(emu):
    nc.run_line(CPU)


def test_refusals_before_any_launch(emu):
    L = emu.lib
    buf = torch.zeros(4096, dtype=torch.int64)
    p = buf.data_ptr()
    K = _lib.ScEngineLib.knn_desc
    for desc, args in [(K(0, 8, 8, 3), (p, p, p, p)), (K(4, 8, 8, 3), (p, p, p, p)), (K(2, -1, 8, 3), (p, p, p, p)),
                       (K(2, 8, -1, 3), (p, p, p, p)), (K(2, 8, 8, 2), (p, p, p, p)), (K(2, 40, 8, 33), (p, p, p, p)),
                       (K(2, 8, 8, 9), (p, p, p, p)), (K(2, 8, 8, 3), (None, p, p, p)), (K(2, 8, 8, 3), (p, None, p, p)),
                       (K(2, 8, 8, 3), (p, p, None, p)), (K(2, 8, 8, 3), (p, p, p, None))]:
        assert L.sc_knn(ctypes.byref(desc), *args, None) != 0
        assert "sc_engine" in L.sc_last_error().decode()
    assert L.sc_knn(None, p, p, p, p, None) != 0
    assert L.sc_knn(ctypes.byref(K(2, 0, 0, 3)), None, None, None, None, None) == 0      # no queries: nothing to do
    N = _lib.ScEngineLib.nufd_desc
    good = dict(n=8, k=4, n_deriv=2, batch=1, d=2, deriv=(0, 1))
    for bad in (dict(n=-1), dict(k=0), dict(k=33), dict(k=2), dict(n_deriv=0), dict(n_deriv=9), dict(d=0), dict(d=4),
                dict(deriv=(0, 2)), dict(deriv=(-1, 0)), dict(radius=-1.0), dict(radius=float("nan")), dict(lam=-1.0),
                dict(d=3, radius=0.5), dict(batch=0)):
        desc = N(**{**good, **bad})
        assert L.sc_nufd_weights(ctypes.byref(desc), p, p, p, p, p, None) != 0, bad
        assert "sc_engine" in L.sc_last_error().decode()
    for bad in (dict(n=-1), dict(k=0), dict(k=33), dict(n_deriv=0), dict(n_deriv=9), dict(batch=0), dict(batch=65536)):
        desc = N(**{**good, **bad})
        assert L.sc_nufd_apply(ctypes.byref(desc), p, p, p, p, None) != 0, bad
        assert L.sc_nufd_apply_adjoint(ctypes.byref(desc), p, p, p, p, p, None) != 0, bad
    ok = N(**good)
    for hole in range(5):
        args = [p] * 5
        args[hole] = None
        if hole != 2:                                        # d2 is read with a radius only
            assert L.sc_nufd_weights(ctypes.byref(ok), *args, None) != 0
        assert L.sc_nufd_apply_adjoint(ctypes.byref(ok), *args, None) != 0
    assert L.sc_nufd_weights(ctypes.byref(N(**{**good, "radius": 0.5})), p, p, None, p, p, None) != 0
    for hole in range(4):
        args = [p] * 4
        args[hole] = None
        assert L.sc_nufd_apply(ctypes.byref(ok), *args, None) != 0
    assert L.sc_nufd_weights(None, p, p, p, p, p, None) != 0
    empty = N(**{**good, "n": 0})                            # a valid empty cloud is no refusal
    assert L.sc_nufd_weights(ctypes.byref(empty), None, None, None, None, None, None) == 0
    assert L.sc_nufd_apply(ctypes.byref(empty), None, None, None, None, None) == 0
    assert L.sc_nufd_apply_adjoint(ctypes.byref(empty), None, None, None, None, None, None) == 0


def test_out_of_range_indices_address_nothing(emu):
    """a caller's stencil with indices outside [0, n): such a neighbour is masked in the weights and skipped by the apply"""
    n, k = 6, 4
    pts = torch.tensor([[0., 0.], [1., 0.], [0., 1.], [1., 1.], [.5, .25], [.25, .75]])
    idx = torch.tensor([[0, 1, 2, 3], [1, 0, -1, 3], [2, 0, 3, 1 << 40], [3, 1, 2, n], [4, 0, 1, 2], [5, 2, 3, 0]])
    d2 = torch.zeros(n, k)
    w = torch.full((n, 1, k), 7.0)
    flag = torch.full((n,), 9, dtype=torch.int32)
    desc = _lib.ScEngineLib.nufd_desc(n=n, k=k, n_deriv=1, d=2, deriv=(0,))
    emu.nufd_weights(desc, pts.data_ptr(), idx.data_ptr(), d2.data_ptr(), w.data_ptr(), flag.data_ptr())
    assert flag.tolist() == [0] * n and bool(torch.isfinite(w).all())
    assert w[1, 0, 2] == 0 and w[2, 0, 3] == 0 and w[3, 0, 3] == 0
    vals = torch.arange(1.0, n + 1).reshape(1, n)
    out = torch.zeros(1, 1, n)
    emu.nufd_apply(desc, w.data_ptr(), idx.data_ptr(), vals.data_ptr(), out.data_ptr())
    safe = idx.clamp(0, n - 1)
    want = (w[:, 0] * vals[0][safe] * ((idx >= 0) & (idx < n))).sum(1)
    assert nr.rel_l2(out[0, 0].numpy(), want.numpy()) < 1e-6
