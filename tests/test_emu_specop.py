"""The spectral-derivative multiplier pass (sc_kernels_specop.h: sc_spectral_op) in host emulation against a float64
numpy evaluation of its own formula with random complex tables: last kept extents 1, 4, 5, 33, 129 (and 300: waves side
by side), row counts 1, 7, 64 (two non-last axes included), groups 1, 5, 33, one to three sources, an output without a
term, both output layouts, conj, a spectrum at an address that is only 8-byte aligned; the adjoint identity; a
bit-identical repeat; sizes, term counts and a table off the operand's device refused before any launch.  The runner
and the float64 formula are those of fourier_diff_reference, shared with the GPU tier
(tests/test_gpu_specop_kernels.py), whose quick cases (EMU_SPECOP_KERNEL_CASES) run here at the same two bars."""
import numpy as np
import pytest
import torch

import fourier_diff_reference as fr
from emu_engine import engine_on_emulation
from engine_runner import rel_l2
from fourier_diff_reference import crandn as _crandn, spec_tables as _tables, spec_terms as _terms, \
    want_spectral_op as _want
from neuraloperator_amd import _lib, engine


# kept, groups, n_src, n_out, n_terms, empty output, conj, out_major
CASES = [((1,), 1, 1, 1, 1, None, False, False),
         ((4,), 5, 2, 2, 3, None, False, True),
         ((5,), 33, 1, 3, 3, 1, True, False),
         ((7, 33), 5, 3, 3, 6, None, False, False),
         ((64, 129), 1, 1, 2, 2, None, False, True),
         ((7, 129), 33, 1, 1, 2, None, True, True),
         ((64, 5), 33, 2, 1, 2, None, False, False),
         ((1, 4), 5, 3, 4, 9, 2, False, True),
         ((8, 8, 33), 5, 3, 3, 6, None, True, False),
         ((7, 1, 1), 1, 1, 9, 9, None, False, True),
         ((3, 300), 5, 2, 2, 12, None, False, False)]


@pytest.mark.parametrize("case", CASES, ids=["x".join(map(str, c[0])) + f"-g{c[1]}-s{c[2]}-o{c[3]}" for c in CASES])
def test_spectral_op_matches_float64(case):
    kept, groups, n_src, n_out, n_terms, empty, conj, out_major = case
    g = torch.Generator().manual_seed(sum(kept) * 100 + groups)
    n_tab = tuple(2 + d for d in range(len(kept)))
    tabs = _tables(g, kept, n_tab)
    terms = _terms(g, n_src, n_out, n_tab, n_terms, empty)
    x = _crandn(g, groups, n_src, *kept)
    with engine_on_emulation():
        y = engine.SpectralOpFn.apply(x, tabs, terms, n_out, conj, out_major)
        y2 = engine.SpectralOpFn.apply(x, tabs, terms, n_out, conj, out_major)
    assert tuple(y.shape) == ((n_out, groups) if out_major else (groups, n_out)) + tuple(kept)
    got = y.transpose(0, 1) if out_major else y
    assert rel_l2(got.numpy(), _want(x, tabs, terms, n_out, conj)) <= 2e-6
    assert torch.equal(torch.view_as_real(y), torch.view_as_real(y2))          # the same bits twice
    if empty is not None:
        assert torch.all(torch.view_as_real(got[:, empty]) == 0)


@pytest.mark.parametrize("kept", [(5,), (64, 129), (7, 33)], ids=["5", "64x129", "7x33"])
def test_spectrum_on_an_8_byte_aligned_address(kept):
    """source and result one complex element into 16-byte aligned storage: every row starts on the other parity"""
    g = torch.Generator().manual_seed(5)
    n_tab = (2,) * len(kept)
    tabs = _tables(g, kept, n_tab)
    terms = _terms(g, 2, 2, n_tab, 4)
    modes = int(np.prod(kept))
    store = _crandn(g, 5 * 2 * modes + 1)
    x = store[1:].view(5, 2, *kept)
    assert x.data_ptr() % 16 == 8 or store.data_ptr() % 16 == 8
    want = _want(x, tabs, terms, 2, False)
    with engine_on_emulation() as lib:
        ybuf = torch.zeros(5 * 2 * modes + 2, dtype=torch.complex64)
        for off in (0, 1):                                   # both parities of the result's address
            y = ybuf[off:off + 5 * 2 * modes].view(5, 2, *kept)
            lib.spectral_op(torch.view_as_real(x).data_ptr(), torch.view_as_real(y).data_ptr(), kept=kept, groups=5,
                            n_src=2, n_out=2, terms=terms, tabs_a=[t.data_ptr() for t in tabs.a],
                            tabs_b=[t.data_ptr() for t in tabs.b], n_tab=n_tab, y_group_stride=2 * modes,
                            y_out_stride=modes)
            assert rel_l2(y.numpy(), want) <= 2e-6
            assert ybuf[off + 5 * 2 * modes] == 0            # nothing past the end


@pytest.mark.parametrize("case", [CASES[3], CASES[8], CASES[1]], ids=["2d", "3d", "1d-out-major"])
def test_adjoint_identity_and_autograd(case):
    """<Op x, y> = <x, Op^H y>, Op^H the call with sources and outputs exchanged and conj; autograd is that call, and
    differentiates twice"""
    kept, groups, n_src, n_out, n_terms, _, conj, out_major = case
    g = torch.Generator().manual_seed(17)
    n_tab = (3,) * len(kept)
    tabs = _tables(g, kept, n_tab)
    terms = _terms(g, n_src, n_out, n_tab, n_terms)
    back = tuple((o, s, c, t) for s, o, c, t in terms)
    x = _crandn(g, groups, n_src, *kept).requires_grad_(True)
    z = _crandn(g, groups, n_src, *kept)
    yshape = ((n_out, groups) if out_major else (groups, n_out)) + tuple(kept)
    y = _crandn(g, *yshape).requires_grad_(True)
    dot = lambda a, b: complex(torch.sum(a.conj() * b))
    with engine_on_emulation():
        ox = engine.EngineOps.spectral_op(x, tabs, terms, n_out, conj, out_major)
        oz = engine.EngineOps.spectral_op(z, tabs, terms, n_out, conj, out_major)
        yg = y.detach().transpose(0, 1).contiguous() if out_major else y.detach()
        ohy = engine.EngineOps.spectral_op(yg, tabs, back, n_src, not conj, False)
        gx, = torch.autograd.grad((ox.conj() * y).real.sum(), x, create_graph=True)
        gy2, = torch.autograd.grad((gx.conj() * z).real.sum(), y)              # through the backward's own graph
    lhs, rhs = dot(y.detach(), ox.detach()), dot(ohy, x.detach())
    assert abs(lhs - rhs) <= 1e-5 * (abs(lhs) + abs(rhs))
    assert rel_l2(gx.detach().numpy(), ohy.numpy()) <= 1e-6                    # d/dx Re<Op x, y> = Op^H y
    assert rel_l2(gy2.resolve_conj().numpy(), oz.numpy()) <= 1e-6                             # d/dy Re<Op^H y, z> = Op z


def test_long_lists_are_split_and_many_sources_are_summed():
    """20 outputs (two launches) and the 20-source backward (summed from launches of three)"""
    g = torch.Generator().manual_seed(23)
    kept, n_tab = (6, 5), (4, 4)
    tabs = _tables(g, kept, n_tab)
    terms = _terms(g, 1, 20, n_tab, 20)
    x = _crandn(g, 3, 1, *kept).requires_grad_(True)
    cot = _crandn(g, 20, 3, *kept)
    with engine_on_emulation():
        y = engine.EngineOps.spectral_op(x, tabs, terms, 20, False, True)
        gx, = torch.autograd.grad((y.conj() * cot).real.sum(), x)
    assert rel_l2(y.detach().transpose(0, 1).numpy(), _want(x.detach(), tabs, terms, 20, False)) <= 2e-6
    back = tuple((o, s, c, t) for s, o, c, t in terms)
    want = _want(cot.transpose(0, 1), tabs, back, 1, True)
    assert rel_l2(gx.numpy(), want) <= 2e-6


def test_bad_sizes_and_term_counts_are_refused():
    g = torch.Generator().manual_seed(1)
    kept, n_tab = (4, 3), (2, 2)
    tabs = _tables(g, kept, n_tab)
    x = _crandn(g, 2, 2, *kept)
    ok = dict(terms=((0, 0, 1.0, (0, 0)), (1, 1, 1.0, (1, 1))))
    with engine_on_emulation() as lib:
        fr.refused_specop_arguments(lib)
        with pytest.raises(ValueError, match="tables for"):
            engine.SpectralOpFn.apply(x[..., :2], tabs, ok["terms"], 2)
        with pytest.raises(ValueError, match="outside"):
            engine.SpectralOpFn.apply(x, tabs, ((0, 0, 1.0, (0, 5)),), 2)
    with pytest.raises(ValueError):
        engine.SpectralTables([tabs.a[0].to(torch.complex128)], [tabs.b[0]])


def test_tables_off_the_operands_device_are_refused(monkeypatch):
    """both pointers reach the kernel: tables on another device must raise before any launch"""
    g = torch.Generator().manual_seed(2)
    tabs = _tables(g, (4,), (1,))
    meta = engine.SpectralTables([t.to("meta") for t in tabs.a], [t.to("meta") for t in tabs.b])
    x = _crandn(g, 2, 1, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.SpectralOpFn.apply(x, tabs, ((0, 0, 1.0, (0,)),), 1)            # the product refuses host operands
    monkeypatch.setattr(engine, "_require_gpu", lambda *a, **k: None)
    monkeypatch.setattr(_lib, "_LIB", None)                                    # a launch would need the library
    with pytest.raises(ValueError, match="spectral tables on"):
        engine.SpectralOpFn.apply(x, meta, ((0, 0, 1.0, (0,)),), 1)


@pytest.mark.parametrize("name", fr.EMU_SPECOP_KERNEL_CASES)
def test_kernel_edge_cases_of_the_gpu_tier(name):
    """the cases of tests/test_gpu_specop_kernels.py the emulation finishes quickly, at the same two bars"""
    cfg = fr.SPECOP_KERNEL_CASES[name]
    inputs = fr.specop_case_inputs(cfg, 91)
    with engine_on_emulation() as lib:
        got = fr.run_specop_case(lib, cfg, inputs)
    fr.check_specop_case(name, cfg, inputs, got)
