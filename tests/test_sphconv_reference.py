"""SURVEY section 8 row f4 against the reference's OWN layer code: the verbatim
neuralop/layers/spherical_convolution.py SphericalConv, its ``torch_harmonics`` import served by
the classes ``neuraloperator_amd.install_torch_harmonics()`` registers (engine in host emulation), against ``neuraloperator_amd.SphericalConv``
given the same weights; and both against the verbatim layer driven by a float64 pure-torch SHT (tests/sht_reference.py),
whose results are the fixtures tests/golden/sphconv_*.npz the GPU tier reads (``SC_RECORD_SPHCONV=1`` rewrites them).

Needs the reference tree (skipped elsewhere) except ``test_golden_fixtures_are_complete``."""
import os

import numpy as np
import pytest
import torch

from emu_engine import engine_on_emulation
from engine_runner import rel_l2
from oracle import ref_verbatim

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (name, factorization, grid, in / out channels, n_modes, input grid, output_shape)
CASES = [("sphconv_dense_eq", "dense", "equiangular", (3, 4), (8, 16), (17, 32), None),
         ("sphconv_dense_lg", "dense", "legendre-gauss", (3, 4), (8, 12), (12, 24), None),
         ("sphconv_cp_eq", "cp", "equiangular", (4, 4), (6, 12), (13, 24), None),
         ("sphconv_cp_lg", "cp", "legendre-gauss", (3, 2), (8, 16), (10, 20), None),
         ("sphconv_dense_eq_res", "dense", "equiangular", (3, 4), (8, 16), (17, 32), (25, 48))]
needs_reference = pytest.mark.skipif(not ref_verbatim.available(), reason="verbatim reference not present")


def _inputs(name, ci, co, grid_in, out_shape):
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    x = torch.randn(2, ci, *grid_in, generator=g)
    g_out = torch.randn(2, co, *(out_shape or grid_in), generator=g)
    return x, g_out


def _run(conv, x, g, out_shape):
    conv.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    y = conv(xi, output_shape=out_shape) if out_shape else conv(xi)
    y.backward(g)
    grads = {n: p.grad.detach().clone() for n, p in conv.named_parameters()}
    return y.detach(), xi.grad.detach(), grads


def _reference_layer(mod, fac, grid, ci, co, n_modes):
    torch.manual_seed(3)
    ref = mod.SphericalConv(ci, co, n_modes, factorization=fac, rank=0.5, sht_grids=grid)
    with torch.no_grad():
        for p in ref.parameters():
            p.mul_(2.0)
    return ref


def _compare(a, b, tol):
    (ya, gxa, gwa), (yb, gxb, gwb) = a, b
    errs = {"y": rel_l2(ya.numpy(), yb.numpy()), "gx": rel_l2(gxa.numpy(), gxb.numpy())}
    for n in gwb:
        errs["g:" + n] = rel_l2(np.asarray(gwa[n].numpy()), np.asarray(gwb[n].numpy()))
    assert set(gwa) == set(gwb)
    assert all(v <= tol for v in errs.values()), errs
    return errs


@needs_reference
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_verbatim_spherical_conv_on_the_shim_matches_ours(case):
    from neuraloperator_amd import SphericalConv
    import sht_reference
    name, fac, grid, (ci, co), n_modes, grid_in, out_shape = case
    x, g = _inputs(name, ci, co, grid_in, out_shape)
    ref64 = sht_reference.load_reference_spherical("float64")
    ref_f64 = _reference_layer(ref64, fac, grid, ci, co, n_modes)
    want = _run(ref_f64, x, g, out_shape)
    mod = sht_reference.load_reference_spherical("engine")
    ref = _reference_layer(mod, fac, grid, ci, co, n_modes)
    ours = SphericalConv(ci, co, n_modes, factorization=fac, rank=0.5, sht_grids=grid)
    ours.load_state_dict(ref.state_dict(), strict=True)
    assert set(ours.state_dict()) == set(ref.state_dict())
    with engine_on_emulation():
        got_ref = _run(ref, x, g, out_shape)
        got = _run(ours, x, g, out_shape)
    _compare(got_ref, got, 1e-5)            # the reference's own layer on the engine's transforms vs ours
    _compare(got, want, 1e-5)               # ours vs the reference layer on a float64 SHT
    path = os.path.join(GOLDEN, name + ".npz")
    if os.environ.get("SC_RECORD_SPHCONV") == "1":
        y, gx, gw = want
        np.savez_compressed(path, x=x.numpy(), g=g.numpy(), y=y.numpy(), gx=gx.numpy(), n_modes=np.array(n_modes),
                            **{"p:" + n: p.detach().numpy() for n, p in ref_f64.state_dict().items()},
                            **{"g:" + n: v.numpy() for n, v in gw.items()})
    rec = dict(np.load(path))
    assert rel_l2(rec["y"], want[0].numpy()) < 1e-6 and rel_l2(rec["gx"], want[1].numpy()) < 1e-6


def test_golden_fixtures_are_complete():
    for case in CASES:
        rec = dict(np.load(os.path.join(GOLDEN, case[0] + ".npz")))
        assert {"x", "g", "y", "gx", "n_modes"} <= set(rec) and any(k.startswith("p:") for k in rec)
        assert {k[2:] for k in rec if k.startswith("g:")} <= {k[2:] for k in rec if k.startswith("p:")}
