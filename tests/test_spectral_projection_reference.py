"""``neuraloperator_amd.spectral_projection`` in the CPU tier against the fixtures recorded from the verbatim reference
function (tests/golden/sproj_*.npz, tests/record_spectral_projection.py): the torch route and the engine route in host
emulation, output and ``u.grad``, at the project's fp32 parity bar 1e-5 (the reference's own fp32 run sits at 0.9 ..
1.3e-7 from its float64 run, recorded as ``err:fp32``, so the bar tests the formula, not the rounding).  Where the
reference exists the float64 helper restatement is held against the verbatim function at 1e-7.  ``HelmholtzProjection``
against its float64 helper in 2-d and 3-d; idempotence, self-adjointness and a vanishing ``FourierDiff`` divergence on
odd and even grids, each at 1e-5 of ``|u|``; the refused descriptors and the error paths."""
import math

import pytest
import torch

import spectral_projection_reference as pr
from emu_engine import engine_on_emulation
from neuraloperator_amd import FourierDiff, HelmholtzProjection, spectral_projection, \
    spectral_projection_divergence_free

needs_reference = pytest.mark.skipif(not pr.reference_available(), reason="the verbatim reference is not on this machine")


def _route_results(name, route):
    grid, domain, modes = pr.CASES[name]
    rec = pr.load_fixture(name)
    u = torch.from_numpy(rec["u"]).requires_grad_(True)
    if route == "engine":
        with engine_on_emulation(), spectral_projection.route("engine"):
            assert spectral_projection.on_engine(u, domain, modes)
            got = pr.run_case(spectral_projection_divergence_free, u, domain, modes, int(rec["gseed"]))
    else:
        with spectral_projection.route("torch"):
            assert not spectral_projection.on_engine(u, domain, modes)
            got = pr.run_case(spectral_projection_divergence_free, u, domain, modes, int(rec["gseed"]))
    return rec, got


@pytest.mark.parametrize("route", ["torch", "engine"])
@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_both_routes_match_the_recorded_reference(name, route):
    rec, got = _route_results(name, route)
    errs = {k: pr.rel_l2(t, rec["ref:" + k]) for k, t in got.items()}
    print(name, route, {k: f"{e:.2e}" for k, e in errs.items()}, f"reference's own fp32 {float(rec['err:fp32']):.1e}")
    assert all(t.dtype == torch.float32 and tuple(t.shape) == rec["ref:" + k].shape for k, t in got.items())
    assert all(e <= 1e-5 for e in errs.values()), errs


@pytest.mark.parametrize("route", ["torch", "engine"])
def test_one_mode_per_axis_gives_exactly_zero(route):
    rec, got = _route_results("sproj_5x8_m1x1_zero", route)
    assert not rec["ref:out"].any() and not rec["ref:grad"].any()
    assert torch.all(got["out"] == 0) and torch.all(got["grad"] == 0)


@needs_reference
@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_helper_fixtures_and_live_reference_agree(name):
    grid, domain, modes = pr.CASES[name]
    rec = pr.load_fixture(name)
    ref = pr.load_reference_projection()
    u = torch.from_numpy(rec["u"]).double().requires_grad_(True)
    with pr.default_float64():
        live = pr.run_case(ref, u, domain, modes, int(rec["gseed"]))
    as_run = pr.run_case(ref, u, domain, modes, int(rec["gseed"]))           # fp32 wavenumbers, as its users run it
    helper = pr.run_case(pr.f64_projection, u, domain, modes, int(rec["gseed"]))
    for k, t in live.items():
        assert pr.rel_l2(t, rec["ref:" + k]) <= 1e-12, k                     # the fixtures are what the reference computes
        assert pr.rel_l2(helper[k], t) <= 1e-7 and pr.rel_l2(helper[k], as_run[k]) <= 1e-7, k


def test_other_dtypes_devices_and_extents_take_the_torch_route():
    """float64, complex and an extent of 1 run the same multiplier in torch and keep the reference's return dtype"""
    g = torch.Generator().manual_seed(2)
    u = torch.randn(2, 2, 8, 6, generator=g, dtype=torch.float64)
    want = pr.f64_projection(u, (1.3, 2.9), (5, 4))
    assert not spectral_projection.on_engine(u, (1.3, 2.9), (5, 4))
    got = spectral_projection_divergence_free(u, (1.3, 2.9), (5, 4))
    assert got.dtype == torch.float64 and pr.rel_l2(got, want) <= 1e-12
    v = torch.randn(2, 2, 8, 6, generator=g, dtype=torch.float64)
    z = torch.complex(u, v)
    gz = spectral_projection_divergence_free(z, (1.3, 2.9), (5, 4))
    mult = pr.f64_multiplier(8, 6, (1.3, 2.9), (5, 4)).to(torch.complex128)
    wz = torch.fft.ifftn(pr.apply_multiplier(mult, torch.fft.fftn(z, dim=(2, 3))), dim=(2, 3)).real
    assert gz.dtype == torch.float64 and pr.rel_l2(gz, wz) <= 1e-12
    for shape in ((2, 2, 1, 8), (2, 2, 8, 1)):
        u1 = torch.randn(*shape, generator=g)
        with engine_on_emulation():                                          # eligible but for the extent
            assert not spectral_projection.on_engine(u1, 1.0, (4, 4))
            got = spectral_projection_divergence_free(u1, 1.0, (4, 4))
        assert got.dtype == torch.float32 and pr.rel_l2(got, pr.f64_projection(u1, 1.0, (4, 4))) <= 1e-5


def test_routes_and_error_paths():
    u = torch.zeros(2, 2, 8, 8)
    with pytest.raises(ValueError, match="domain_size must be a number or a"):
        spectral_projection_divergence_free(u, "1.0", (4, 4))
    with pytest.raises(ValueError, match="domain_size must be a number or a"):
        spectral_projection_divergence_free(u, (1.0, 2.0, 3.0), (4, 4))
    with pytest.raises(ValueError, match="2 components"):
        spectral_projection_divergence_free(torch.zeros(2, 3, 8, 8), 1.0, (4, 4))
    with pytest.raises(ValueError, match="route must be one of"):
        with spectral_projection.route("hip"):
            pass
    with spectral_projection.route("engine"):
        with pytest.raises(ValueError, match="not eligible"):                # a host tensor: the engine has no CPU path
            spectral_projection_divergence_free(u, 1.0, (4, 4))
        with pytest.raises(ValueError, match="not eligible"):
            HelmholtzProjection(2)(u)
    with engine_on_emulation():
        with spectral_projection.route("engine"):
            assert spectral_projection.on_engine(u, 1.0, (4, 4)) and HelmholtzProjection(2).on_engine(u)
            assert not spectral_projection.on_engine(u.double(), 1.0, (4, 4))
            assert not spectral_projection.on_engine(u, None, (4, 4))
        with spectral_projection.route("torch"):
            assert not spectral_projection.on_engine(u, 1.0, (4, 4)) and not HelmholtzProjection(2).on_engine(u)
        assert spectral_projection.on_engine(u, 1.0, (4, 4)) == spectral_projection.AUTO_TAKES_ENGINE
    with pytest.raises(ValueError, match="dim must be 2 or 3"):
        HelmholtzProjection(1)
    with pytest.raises(ValueError, match="L must be a single float or tuple with 2 elements"):
        HelmholtzProjection(2, L=(1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match="constraint_modes"):
        HelmholtzProjection(2, constraint_modes=(4, 0))
    with pytest.raises(ValueError, match="input must be"):
        HelmholtzProjection(3)(torch.zeros(2, 2, 4, 4, 4))


# leading + component + spatial shape, L, constraint_modes
CLASS_CASES = [((2, 2, 8, 10), None, None), ((3, 2, 7, 9), (1.3, 2.9), (5, 4)), ((2, 2, 16, 12), 2.0, 6),
               ((2, 3, 6, 5, 8), None, None), ((1, 2, 3, 8, 12, 10), (1.5, 0.9, 2.6), (5, 7, 4))]


@pytest.mark.parametrize("route", ["torch", "engine"])
@pytest.mark.parametrize("case", CLASS_CASES, ids=["x".join(map(str, c[0])) for c in CLASS_CASES])
def test_helmholtz_projection_matches_its_float64_helper(case, route):
    shape, L, modes = case
    dim = 2 if shape[-3] == 2 and len(shape) == 4 else 3
    g = torch.Generator().manual_seed(sum(shape))
    u = torch.randn(*shape, generator=g).requires_grad_(True)
    cot = torch.randn(*shape, generator=g)
    P = HelmholtzProjection(dim, L=L, constraint_modes=modes)
    if route == "engine":
        with engine_on_emulation(), spectral_projection.route("engine"):
            assert P.on_engine(u)
            y = P(u)
            gu, = torch.autograd.grad((y * cot).sum(), u)
    else:
        with spectral_projection.route("torch"):
            y = P(u)
            gu, = torch.autograd.grad((y * cot).sum(), u)
    u64 = u.detach().double().requires_grad_(True)
    y64 = pr.f64_helmholtz(u64, dim, L, modes)
    g64, = torch.autograd.grad((y64 * cot.double()).sum(), u64)
    assert y.dtype == torch.float32 and y.shape == u.shape
    assert pr.rel_l2(y.detach(), y64.detach()) <= 1e-5 and pr.rel_l2(gu, g64) <= 1e-5


@pytest.mark.parametrize("modes", [None, 5], ids=["all-modes", "low-pass"])
@pytest.mark.parametrize("grid", pr.PROPERTY_GRIDS, ids=["x".join(map(str, s)) for s in pr.PROPERTY_GRIDS])
def test_projection_properties_on_odd_and_even_grids(grid, modes):
    dim = len(grid)
    g = torch.Generator().manual_seed(sum(grid))
    u, v = torch.randn(3, dim, *grid, generator=g), torch.randn(3, dim, *grid, generator=g)
    P = HelmholtzProjection(dim, constraint_modes=modes)
    with engine_on_emulation(), spectral_projection.route("engine"):
        got = pr.properties(P, FourierDiff(dim), u, v)
    print(grid, modes, "idempotence %.1e self-adjointness %.1e divergence %.1e" % got)
    assert max(got) <= 1e-5, got


@pytest.mark.parametrize("name", sorted(pr.CASES))
def test_the_reference_function_is_its_own_adjoint(name):
    grid, domain, modes = pr.CASES[name]
    g = torch.Generator().manual_seed(5)
    u, v = torch.randn(2, 2, *grid, generator=g), torch.randn(2, 2, *grid, generator=g)
    with engine_on_emulation(), spectral_projection.route("engine"):
        pu = spectral_projection_divergence_free(u, domain, modes)
        pv = spectral_projection_divergence_free(v, domain, modes)
    lhs, rhs = float((pu.double() * v).sum()), float((u.double() * pv).sum())
    assert abs(lhs - rhs) <= 1e-5 * float(u.norm()) * float(v.norm())


def test_double_backward():
    """the backward pass is the operator itself, so autograd differentiates it again"""
    g = torch.Generator().manual_seed(4)
    u = torch.randn(2, 2, 7, 6, generator=g).requires_grad_(True)
    c = torch.randn(2, 2, 7, 6, generator=g).requires_grad_(True)
    with engine_on_emulation(), spectral_projection.route("engine"):
        y = spectral_projection_divergence_free(u, (1.3, 0.7), (5, 4))
        gu, = torch.autograd.grad((y * c).sum(), u, create_graph=True)
        gc, = torch.autograd.grad(gu.square().sum(), c)
    u64, c64 = u.detach().double().requires_grad_(True), c.detach().double().requires_grad_(True)
    gu64, = torch.autograd.grad((pr.f64_projection(u64, (1.3, 0.7), (5, 4)) * c64).sum(), u64, create_graph=True)
    gc64, = torch.autograd.grad(gu64.square().sum(), c64)
    assert pr.rel_l2(gu.detach(), gu64.detach()) <= 1e-5 and pr.rel_l2(gc, gc64) <= 1e-5


def test_pruned_blocks_hold_the_kept_frequencies_and_their_mirrors():
    """the transform pair is pruned where the crop keeps fewer modes than the grid has"""
    from neuraloperator_amd import engine
    seen = []
    u = torch.randn(1, 2, 32, 40, generator=torch.Generator().manual_seed(1))
    with engine_on_emulation(), spectral_projection.route("engine"):
        for modes in ((32, 40), (8, 8), (7, 9), (32, 6), (31, 39)):
            got = spectral_projection_divergence_free(u, 1.0, modes)
            assert pr.rel_l2(got, pr.f64_projection(u, 1.0, modes)) <= 1e-5, modes
            seen.append(list(engine._HELM_TABLES.values())[-1].kept)        # the most recently used tables
    # (8, 8): frequencies -4 .. 3 and the mirror +4: p = 4; (7, 9): -4 .. 2 / -5 .. 3 (the off-by-one), p = 4 / 5;
    # (31, 39): p = 16 / 20 would keep the whole axis
    assert seen == [(32, 21), (9, 5), (9, 6), (32, 4), (32, 21)]


def test_refused_descriptors_return_their_errors():
    with engine_on_emulation() as lib:
        pr.refused_helmholtz_arguments(lib)


def test_default_length_is_two_pi():
    assert HelmholtzProjection(2).L == (2 * math.pi,) * 2 and HelmholtzProjection(3, L=1.5).L == (1.5,) * 3
