"""GPU tier: the spectral-derivative multiplier pass (sc_kernels_specop.h: k_spectral_op) at its wave-layout, group and
grid edges on an MI355X, driven through the C-ABI with free-standing descriptors (fourier_diff_reference.run_spectral_op)
against a float64 numpy evaluation of the kernel's own formula with random complex tables.  SPECOP_KERNEL_CASES:
  a  last kept extent 1, 2, 127 .. 129, 255 .. 257, 511 .. 513, 1025 with 3 rows and 5 groups: one, two and four waves
     side by side, a second column tile at 513; odd extents alternate the rows' alignment
  b  groups per workgroup: one row of 5 modes with 1 .. 33 groups (gpw falls to 1); 64 x 129 with 257 groups (two waves,
     gpw 8, the last workgroup holds one group); 64 x 257 with 67 groups (four waves, gpw 2, odd group count)
  c  the grid limit: kept (2,) with 8 * 65535 + 1 groups, gpw grows to 16.  The second growth condition (2^23
     workgroups) needs a spectrum above 0.5 GB and is left out.
  d  twelve slots over three sources, a term-less output, conj, out-major strides, kept (5, 6, 7) with two row axes,
     several table rows per axis
  e  xhat and yhat in turn one complex element into 16-byte aligned storage
Every result meets the project's rel-L2 (1e-5) and, per component of every element, |got - want| <= gamma_N A with A
and N from fourier_diff_reference.spectral_op_bound (derived from the kernel source, not measured); a term-less output
(A = 0) is exactly 0, and the sentinel values around the result stay untouched."""
import numpy as np
import pytest
import torch

import fourier_diff_reference as fr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _lib():
    from neuraloperator_amd import _lib
    return _lib.get_lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("name", sorted(fr.SPECOP_KERNEL_CASES))
def test_spectral_op_edges_against_float64(name):
    cfg = fr.SPECOP_KERNEL_CASES[name]
    inputs = fr.specop_case_inputs(cfg, 91)
    got = fr.run_specop_case(_lib(), cfg, inputs, DEV, _stream())
    fr.check_specop_case(name, cfg, inputs, got)


def test_the_plans_the_cases_are_cut_for():
    """(waves side by side as a power of two, column tiles, groups per workgroup, workgroups along the groups) as the
    host's dispatch chooses them: what groups a, b and c are about"""
    plan = {k: fr.specop_plan(c["kept"], c["groups"]) for k, c in fr.SPECOP_KERNEL_CASES.items()}
    assert [plan[f"a_3x{kl}_g5"][:2] for kl in (128, 129, 256, 257, 512, 513, 1025)] == \
        [(0, 1), (1, 1), (1, 1), (2, 1), (2, 1), (2, 2), (2, 3)]
    assert all(plan[f"b_5_g{g}"][2:] == (1, g) for g in (1, 2, 3, 4, 5, 7, 8, 9, 33))
    assert plan["b_64x129_g257_two_waves_gpw8"] == (1, 1, 8, 33)           # 32 workgroups of 8 groups and one of 1
    assert plan["b_64x257_g67_four_waves_gpw2"] == (2, 1, 2, 34)           # 33 workgroups of 2 groups and one of 1
    assert plan["c_2_g524281_gpw16"] == (0, 1, 16, 32768)                  # 65536 workgroups of 8 exceed the grid


@pytest.mark.parametrize("name", ["a_3x129_g5", "a_3x257_g5", "a_3x513_g5", "b_5_g9", "b_64x129_g257_two_waves_gpw8",
                                  "b_64x257_g67_four_waves_gpw2", "c_2_g524281_gpw16", "e_3x129_yhat_off_by_one"])
def test_spectral_op_twice_gives_the_same_bits(name):
    cfg = fr.SPECOP_KERNEL_CASES[name]
    inputs = fr.specop_case_inputs(cfg, 92)
    (a, _), (b, _) = (fr.run_specop_case(_lib(), cfg, inputs, DEV, _stream()) for _ in range(2))
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def test_refused_arguments_return_their_error_on_the_device_library():
    fr.refused_specop_arguments(_lib(), DEV)
