"""GPU tier: the kernels behind factorization="Tucker" | "CP" | "TT" (sc_kernels_tucker.h, sc_kernels_fmx.h,
k_modegemm_msum of sc_kernels_generic.h) at their tile, rank and chunk edges on an MI355X.  Every row of the tables of
factor_reference.py asserts the route it reaches (sc_tucker_modes_path, sc_modegemm_path, sc_modegemm_msum_path), runs
through the C-ABI on buffers between NaN guard bands compared bit for bit, and is held at the project's rel-L2 bar and,
element by element, at gamma_N S with N counted in the kernel source.  Then: refused shapes fail loudly
and write nothing, bit-identical repeats of every fixed-order path, exact zeros from a zero operand on each matrix-core
kernel.  The last test prints the worst |err| / bound per kernel and instantiation."""
import pytest
import torch

import factor_reference as fr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WORST = {}                     # (kernel, tensor) -> (worst element ratio, row)
# The tables are read while pytest collects.  Beside a helper without them this module still has to collect -- an error
# here would stop the collection of every other module of the suite -- and test_the_helper_holds_the_tables fails.
TUCKER = getattr(fr, "TUCKER_CASES", {})
REFUSED = getattr(fr, "TUCKER_REFUSED", {})
BFAC = getattr(fr, "BFAC_CASES", {})
MSUM = getattr(fr, "MSUM_CASES", {})
SLOT = getattr(fr, "SLOT_CASES", {})


def test_the_helper_holds_the_tables():
    assert len(TUCKER) >= 36 and len(REFUSED) == 3 and len(BFAC) >= 55 and len(MSUM) >= 24 and len(SLOT) >= 10
    assert TUCKER is fr.TUCKER_CASES and BFAC is fr.BFAC_CASES and MSUM is fr.MSUM_CASES and SLOT is fr.SLOT_CASES
    cov = fr.coverage()                                  # every path code, instantiation and slot tile has a row
    assert set(p for k, p in cov if k == "tucker") == set(fr.TUCKER_PATHS)


def _lib():
    from neuraloperator_amd import _lib as L
    return L.get_lib()


def _cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def _note(kind, name, stats):
    labels = fr.kernel_labels(kind, name)
    for key, (_, ratio) in stats.items():
        if ratio > WORST.get((labels[key], key), (-1.0, ""))[0]:
            WORST[(labels[key], key)] = (ratio, name)


@pytest.mark.parametrize("name", sorted(TUCKER))
def test_tucker_mode_factors_on_guarded_buffers(name):
    _, stats = fr.run_tucker(_lib(), name, DEV)
    assert set(stats) == {"t", "gcore", "gux", "guy"}
    _note("tucker", name, stats)


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_shapes_fail_loudly_and_write_nothing(name):
    fr.run_tucker_refused(_lib(), name, DEV)


@pytest.mark.parametrize("name", sorted(BFAC))
def test_factor_operand_on_guarded_buffers(name):
    _, stats = fr.run_bfac(_lib(), name, DEV, cus=_cus())
    _note("bfac", name, stats)


@pytest.mark.parametrize("name", sorted(MSUM))
def test_mode_summed_on_the_matrix_cores(name):
    _, stats = fr.run_msum(_lib(), "msum", name, DEV)
    _note("msum", name, stats)


@pytest.mark.parametrize("name", sorted(SLOT))
def test_mode_summed_slot_form(name):
    _, stats = fr.run_msum(_lib(), "slot", name, DEV)
    _note("slot", name, stats)


@pytest.mark.parametrize("name", ["robin_fg1030", "bwd_rx_49", "robin_fg513_vector"])
def test_tucker_repeats_are_bit_identical(name):
    """the backward pass on both routes (both matrix-core instantiations, three slices per workgroup; the vector kernels
    with two): partials reduced in a fixed order"""
    assert {fr.TUCKER_CASES[n]["path"] for n in ("robin_fg1030", "bwd_rx_49", "robin_fg513_vector")} == {11, 12, 1}
    lib = _lib()
    a, _ = fr.run_tucker(lib, name, DEV)
    b, _ = fr.run_tucker(lib, name, DEV)
    assert all(torch.equal(a[k], b[k]) for k in ("t", "gcore", "gux", "guy"))


@pytest.mark.parametrize("kind,name", [("msum", "chunks_1100"), ("msum", "i9164_P36_Q49"), ("slot", "reduce_n65"),
                                       ("slot", "P65_wide")])
def test_mode_summed_repeats_are_bit_identical(kind, name):
    """sc_modegemm_msum_ws on both routes (the atomic form is not reproducible and not part of this)"""
    lib = _lib()
    a, _ = fr.run_msum(lib, kind, name, DEV)
    b, _ = fr.run_msum(lib, kind, name, DEV)
    assert torch.equal(a, b)


def test_factor_operand_repeats_are_bit_identical_over_uneven_rounds():
    lib = _lib()
    a, _ = fr.run_bfac(lib, fr.BFAC_UNEVEN, DEV, cus=_cus())
    b, _ = fr.run_bfac(lib, fr.BFAC_UNEVEN, DEV, cus=_cus())
    assert torch.equal(a, b)


@pytest.mark.parametrize("name", ["tiles_37_19_63_33", "bwd_ry_33", "fwd_4_4", "fwd_16_3_small_m", "fwd_16_4"])
def test_a_zero_operand_gives_exact_zeros_on_the_tucker_matrix_core_kernels(name):
    """a zero core: t and both factor gradients exactly zero; a zero cotangent: every gradient exactly zero"""
    assert {fr.TUCKER_CASES[n]["path"] for n in ("tiles_37_19_63_33", "bwd_ry_33", "fwd_4_4", "fwd_16_3_small_m", "fwd_16_4")} \
        == {11, 12, 22, 32, 42}
    lib = _lib()
    core, ux, uy, gt = fr.tucker_inputs(name)
    out, _ = fr.run_tucker(lib, name, DEV, inputs=(torch.zeros_like(core), ux, uy, gt))
    assert all(bool((out[k] == 0).all()) for k in ("t", "gux", "guy")) and bool(torch.isfinite(torch.view_as_real(out["gcore"])).all())
    out, _ = fr.run_tucker(lib, name, DEV, inputs=(core, ux, uy, torch.zeros_like(gt)))
    assert all(bool((out[k] == 0).all()) for k in ("gcore", "gux", "guy"))


@pytest.mark.parametrize("name", ["conj00_R36_Q48", "conj01_R36_Q49", "conj10_R37_Q48", "conj11_R37_Q49"])
def test_a_zero_factor_gives_exact_zeros_on_every_factor_operand_instantiation(name):
    c = fr.BFAC_CASES[name]
    assert fr.bfac_instance(c["R"], c["Q"]) == dict(zip(("conj00_R36_Q48", "conj01_R36_Q49", "conj10_R37_Q48", "conj11_R37_Q49"),
                                                        fr.BFAC_INSTANCES))[name]
    a, b = fr.fmx_inputs("bfac", name)
    got, _ = fr.run_bfac(_lib(), name, DEV, inputs=(a, torch.zeros_like(b)))
    assert bool((got == 0).all())


@pytest.mark.parametrize("name", ["i1693_P64_Q36", "i9164_P36_Q49", "i16164_P37_Q49"])
def test_a_zero_operand_gives_exact_zeros_on_every_mode_summed_instantiation(name):
    c = fr.MSUM_CASES[name]
    assert fr.msum_instance(c["P"], c["Q"]) == dict(zip(("i1693_P64_Q36", "i9164_P36_Q49", "i16164_P37_Q49"), fr.MSUM_INSTANCES))[name]
    a, b = fr.fmx_inputs("msum", name)
    got, _ = fr.run_msum(_lib(), "msum", name, DEV, inputs=(torch.zeros_like(a), b))
    assert bool((got == 0).all())


def test_report_the_worst_ratio_per_kernel():
    """prints, per kernel instantiation and tensor, the worst |err| / (gamma_N S) and the row that produced it (the
    figures of DESIGN 3.29)"""
    for (kernel, key), (ratio, name) in sorted(WORST.items()):
        print(f"{kernel:36s} {key:6s} worst |err| / (gamma_N S) {ratio:.4f} ({name})")
