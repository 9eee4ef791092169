"""GPU tier: the Legendre kernels of the spherical-harmonic transforms (sc_kernels_sht.h: k_legendre_analysis /
k_legendre_synthesis; 4 lines per lane, 16 output rows per workgroup, 4 per wave, 64 columns, 8 terms per step) at their
line, row, step and column-group edges on an MI355X, driven through the C-ABI (sht_reference.run_legendre) against a
float64 einsum with the same fp32 table.  SHT_KERNEL_CASES:
  a  a covering set of lines 1, 3, 4, 5; output rows 1, 3, 4, 5, 15, 16, 17, 33; summed extents 1, 7, 8, 9, 17; mmax 1,
     63, 64, 65, 129 on either side of lmax; random tables whose triangle l < m is exactly zero (the kernels skip it: a
     table with anything there is outside the contract) and the real Legendre tables of sht_reference
  b  synthesis with mmax 65 and 129 and lmax 64, 65, 71, 72, 73, 130: the sum of a later column group starts at
     l = 64 or 128, with a tail that is no multiple of 8, or at / past lmax, where the output is exactly zero
Both kernels run on every case.  Every result meets the project's rel-L2 (1e-5) and, per component of every element,
|got - want| <= gamma_N A with N = summed extent + 1 (sht_reference.legendre_roundings) and A the contraction of the
absolute values; where A is 0 -- the analysis output for l < m, diagonal blocks included, and the synthesis output of
columns m >= lmax -- the value is exactly 0.  The adjoint identity of the two kernels holds on the device."""
import numpy as np
import pytest
import torch

import sht_reference as sr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _lib():
    from neuraloperator_amd import _lib
    return _lib.get_lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("name", sorted(sr.SHT_KERNEL_CASES))
def test_legendre_kernels_edges_against_float64(name):
    inputs = sr.sht_case_inputs(name, 91)
    sr.check_sht_case(name, inputs, sr.run_sht_case(_lib(), inputs, DEV, _stream()))


@pytest.mark.parametrize("name", sr.ADJOINT_CASES)
def test_adjoint_identity_on_the_device(name):
    """<A x, c> = <x, A^T c>: analysis with T and synthesis with the same T"""
    x, c, ta, ts = sr.sht_case_inputs(name, 95)
    dot = lambda a, b: float(torch.sum(a.conj() * b).real.double())
    for tab in (ta, ts):
        ax = sr.run_legendre(_lib(), "analysis", x, tab, DEV, _stream())
        atc = sr.run_legendre(_lib(), "synthesis", c, tab, DEV, _stream())
        lhs, rhs = dot(ax.to(torch.complex128), c.to(torch.complex128)), dot(x.to(torch.complex128), atc.to(torch.complex128))
        print(name, lhs, rhs)
        assert abs(lhs - rhs) <= 1e-5 * (abs(lhs) + abs(rhs))


@pytest.mark.parametrize("name", ["a_L5_9x5x65_random", "a_L3_17x33x63_real", "b_L2_5x73x65_random",
                                  "b_L2_5x130x129_random"])
def test_legendre_kernels_twice_give_the_same_bits(name):
    inputs = sr.sht_case_inputs(name, 92)
    a, b = (sr.run_sht_case(_lib(), inputs, DEV, _stream()) for _ in range(2))
    assert all(torch.equal(torch.view_as_real(p), torch.view_as_real(q)) for p, q in zip(a, b))


def test_refused_arguments_return_their_error_on_the_device_library():
    sr.refused_legendre_arguments(_lib(), DEV)
