"""The per-mode projector pass of the divergence-free projection (sc_kernels_helmholtz.h: sc_helmholtz_project) in host
emulation against a float64 numpy evaluation of its own formula with random tables, through the C-ABI with
free-standing descriptors between sentinel guard bands (spectral_projection_reference.run_helmholtz).  The cases are
those of the GPU tier (tests/test_gpu_helmholtz_kernels.py, HELMHOLTZ_KERNEL_CASES), at the same two bars: rel-L2 1e-5
and, per real component of every element, |got - want| <= gamma_N A with N = 3 n_comp + 2 counted from the kernel
source.  A subset twice for the same bits; bad tables, and tables off the operand's device, refused."""
import pytest
import torch

import spectral_projection_reference as pr
from emu_engine import engine_on_emulation
from neuraloperator_amd import _lib, engine


@pytest.mark.parametrize("name", sorted(pr.HELMHOLTZ_KERNEL_CASES))
def test_kernel_cases_against_float64(name):
    cfg = pr.HELMHOLTZ_KERNEL_CASES[name]
    inputs = pr.helm_case_inputs(cfg, 91)
    with engine_on_emulation() as lib:
        got = pr.run_helm_case(lib, cfg, inputs)
    pr.check_helm_case(name, cfg, inputs, got)


def test_the_plans_the_cases_are_cut_for():
    pr.check_case_plans()


@pytest.mark.parametrize("name", [n for n in pr.REPEAT_CASES if "g257" not in n])
def test_twice_gives_the_same_bits(name):
    cfg = pr.HELMHOLTZ_KERNEL_CASES[name]
    inputs = pr.helm_case_inputs(cfg, 92)
    with engine_on_emulation() as lib:
        (a, _), (b, _) = (pr.run_helm_case(lib, cfg, inputs) for _ in range(2))
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))


def test_bad_tables_and_fields_are_refused():
    g = torch.Generator().manual_seed(3)
    t = pr.helm_tables(g, (4, 3))
    for bad in ((t, (0, 2), pr.EPS), (t, (0,), pr.EPS), (t, (0, 1), 0.0), ([t[0].double(), t[1]], (0, 1), pr.EPS),
                ([t[0]], (0,), pr.EPS), ([t[0][:, :, :2].contiguous(), t[1]], (0, 1), pr.EPS)):
        with pytest.raises(ValueError):
            engine.HelmholtzTables(*bad)
    tabs = engine.HelmholtzTables(t, (0, 1), pr.EPS)
    with engine_on_emulation():
        for shape in ((2, 3, 4, 4), (2, 2, 4), (2, 2, 4, 4, 4)):               # components or dims against the tables
            with pytest.raises(ValueError, match="against helmholtz tables"):
                engine.HelmholtzProjectFn.apply(torch.zeros(*shape), tabs)


def test_tables_off_the_operands_device_are_refused(monkeypatch):
    """both pointers reach the kernel: tables on another device must raise before any launch"""
    g = torch.Generator().manual_seed(2)
    t = pr.helm_tables(g, (4, 3))
    tabs = engine.HelmholtzTables(t, (0, 1), pr.EPS)
    meta = engine.HelmholtzTables([x.to("meta") for x in t], (0, 1), pr.EPS)
    u = torch.zeros(2, 2, 4, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.HelmholtzProjectFn.apply(u, tabs)                               # the product refuses host operands
    monkeypatch.setattr(engine, "_require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(_lib, "_LIB", None)                                    # a launch would need the library
    with pytest.raises(ValueError, match="helmholtz tables on"):
        engine.HelmholtzProjectFn.apply(u, meta)
