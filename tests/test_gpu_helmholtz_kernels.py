"""GPU tier: the per-mode projector pass of the divergence-free projection (sc_kernels_helmholtz.h:
k_helmholtz_project) at its wave-layout, group and alignment edges on an MI355X, driven through the C-ABI with
free-standing descriptors (spectral_projection_reference.run_helmholtz) against a float64 numpy evaluation of the
kernel's own formula.  Tables are random: kappa of both signs, keep and z random 0 / 1, and mode (0, .., 0) of every case
has all K = 0 and w = 1, so eps alone stands in its denominator.  HELMHOLTZ_KERNEL_CASES:
  a  last kept extent 1, 2, 127, 128, 129, 257, 513 with 3 rows and 5 groups: one, two and four waves side by side, a
     second column tile at 513; odd extents alternate the rows' alignment
  b  groups per workgroup: one row of 5 modes with 1 .. 33 groups (gpw 1); 64 x 129 with 257 groups (two waves, gpw 8,
     the last workgroup holds one group)
  c  ndim 3 with kept (5, 6, 7), three components and sel a non-identity permutation; ndim 2 with sel (1, 0) and (0, 0)
  d  in place (yhat == xhat); group-major and component-major strides; xhat and yhat in turn one complex element into
     16-byte aligned storage
  e  keep all zero: the output is exactly zero and the guards are untouched
Every result meets the project's rel-L2 (1e-5) and, per real component of every element, |got - want| <= gamma_N A
with A and N = 3 n_comp + 2 from spectral_projection_reference.helmholtz_bound (derived from the kernel source, not
measured); an element with A = 0 is exactly 0, and the sentinel values around the result stay untouched."""
import pytest
import torch

import spectral_projection_reference as pr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _lib():
    from neuraloperator_amd import _lib
    return _lib.get_lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("name", sorted(pr.HELMHOLTZ_KERNEL_CASES))
def test_helmholtz_edges_against_float64(name):
    cfg = pr.HELMHOLTZ_KERNEL_CASES[name]
    inputs = pr.helm_case_inputs(cfg, 91)
    got = pr.run_helm_case(_lib(), cfg, inputs, DEV, _stream())
    pr.check_helm_case(name, cfg, inputs, got)


def test_the_plans_the_cases_are_cut_for():
    """(waves side by side as a power of two, column tiles, groups per workgroup, workgroups along the groups) as the
    host's dispatch chooses them: what groups a and b are about"""
    pr.check_case_plans()


@pytest.mark.parametrize("name", pr.REPEAT_CASES)
def test_helmholtz_twice_gives_the_same_bits(name):
    cfg = pr.HELMHOLTZ_KERNEL_CASES[name]
    inputs = pr.helm_case_inputs(cfg, 92)
    (a, _), (b, _) = (pr.run_helm_case(_lib(), cfg, inputs, DEV, _stream()) for _ in range(2))
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def test_refused_arguments_return_their_error_on_the_device_library():
    pr.refused_helmholtz_arguments(_lib(), DEV)
