"""CPU tier: the point-cloud finite differences against the fixtures recorded from the verbatim reference
(tests/record_nufd.py -> tests/golden/nufd_*.npz): the helper's closed form, the package's torch route, the engine route
on the emulation library, and the public interface (signatures, clamp, shapes, dtypes, routes, on_engine)."""
import inspect

import numpy as np
import pytest
import torch

import nufd_reference as nr
import neuraloperator_amd
from emu_engine import engine_on_emulation
from neuraloperator_amd import differentiation as D

NAMES = sorted(nr.CASES)


def _kw(cfg):
    return dict(num_neighbors=cfg["k"], derivative_indices=cfg["deriv"], radius=cfg["radius"], regularize_lstsq=cfg["reg"])


@pytest.mark.parametrize("name", NAMES)
def test_closed_form_is_what_the_reference_computes(name):
    cfg = nr.CASES[name]
    ref, (points, values, g) = nr.fixture_results(name)
    inc = ~ref["excluded"]
    assert ref["excluded"].mean() <= nr.MAX_EXCLUDED
    idx, _, _, w = nr.closed_form(points, cfg["k"], cfg["deriv"], cfg["radius"], nr.LAMBDA if cfg["reg"] else 0.0)
    assert nr.same_sets(idx[inc], ref["indices"][inc]).all()
    # a fixture whose weights are stored rounded to fp32 (the size limit) is met to that rounding, 2^-24
    bar = 1e-10 if ref["weights"].dtype == np.float64 else 2.0 ** -24
    e_w = nr.rel_l2(nr.match_by_index(idx[inc], w[inc], ref["indices"][inc]), ref["weights"][inc])
    w = np.where(inc[:, None, None], w, 0.0)
    e_d = nr.rel_l2(nr.apply(w, idx, values)[..., inc], ref["derivatives"][..., inc])
    e_g = nr.rel_l2(nr.adjoint(w, idx, g), ref["grad"])
    print(f"{name}: weights {e_w:.1e} derivatives {e_d:.1e} grad {e_g:.1e}")
    assert e_w <= bar and e_d <= 1e-10 and e_g <= 1e-10


@pytest.mark.parametrize("name", NAMES)
def test_torch_route_matches_the_fixtures(name):
    """float64 CPU tensors run the reference's chain of torch calls: the recorded numbers again"""
    cfg = nr.CASES[name]
    ref, (points, values, g) = nr.fixture_results(name)
    inc = ~ref["excluded"]
    p = torch.from_numpy(points).double()
    v = torch.from_numpy(values[0]).double().requires_grad_()
    assert not D.on_engine(p, v, **_kw(cfg))
    idx, w = D.get_non_uniform_fd_weights(p, **_kw(cfg))
    assert idx.dtype == torch.int64 and w.dtype == torch.float64
    assert idx.shape == (cfg["n"], cfg["k"]) and w.shape == (cfg["n"], len(cfg["deriv"]), cfg["k"])
    der = D.non_uniform_fd(p, v, **_kw(cfg))
    assert der.shape == (len(cfg["deriv"]), cfg["n"])
    der.backward(torch.from_numpy(g[:, 0]).double())
    fd = D.NonUniformFD(p, **_kw(cfg))
    assert not fd.on_engine(v) and fd.k == cfg["k"] and fd.ill_posed().numel() == 0
    batched = fd(torch.stack([v.detach(), 2 * v.detach()]).reshape(2, 1, -1))
    assert batched.shape == (len(cfg["deriv"]), 2, 1, cfg["n"])
    assert nr.same_sets(idx.numpy()[inc], ref["indices"][inc]).all()
    wbar = 1e-8 if ref["weights"].dtype == np.float64 else 2.0 ** -24
    assert nr.rel_l2(nr.match_by_index(idx.numpy()[inc], w.numpy()[inc], ref["indices"][inc]), ref["weights"][inc]) <= wbar
    assert nr.rel_l2(der.detach().numpy()[:, inc], ref["derivatives"][:, 0][:, inc]) <= 1e-8
    assert nr.rel_l2(batched[:, 1, 0].numpy()[:, inc], 2 * ref["derivatives"][:, 0][:, inc]) <= 1e-8
    assert nr.rel_l2(v.grad.numpy(), ref["grad"][0]) <= 1e-8


@pytest.mark.parametrize("name", NAMES)
def test_engine_route_on_emulation_matches_the_fixtures(name):
    cfg = nr.CASES[name]
    ref, (points, values, g) = nr.fixture_results(name)
    p = torch.from_numpy(points)
    v = torch.from_numpy(values[0]).requires_grad_()
    with engine_on_emulation(), D.route("engine"):
        assert D.on_engine(p, v, **_kw(cfg))
        fd = D.NonUniformFD(p, **_kw(cfg))
        assert fd.on_engine(v) and fd.k == cfg["k"]
        der = fd(v)
        der.backward(torch.from_numpy(g[:, 0]))
        assert fd.indices.dtype == torch.int64 and fd.fd_weights.dtype == torch.float32 and der.dtype == torch.float32
        assert der.shape == (len(cfg["deriv"]), cfg["n"])
        assert not set(fd.ill_posed().tolist()) - set(np.nonzero(ref["excluded"])[0].tolist())
        nr.check(name, ref, values, cfg["k"], fd.indices.numpy(), fd._stencil.d2.numpy(), fd.fd_weights.numpy(),
                 der.detach().numpy()[:, None], v.grad.numpy()[None])
        if name == "n300_d2_k5":                             # the two functions and a batch of fields: the same numbers
            idx, w = D.get_non_uniform_fd_weights(p, **_kw(cfg))
            assert torch.equal(idx, fd.indices) and torch.equal(w, fd.fd_weights)
            assert torch.equal(D.non_uniform_fd(p, v.detach(), **_kw(cfg)), der.detach())
            many = fd(torch.stack([v.detach(), -v.detach()]).reshape(2, 1, -1))
            assert many.shape == (2, 2, 1, cfg["n"]) and torch.equal(many[:, 0, 0], der.detach())


def test_public_interface():
    ref_sig = "(points, num_neighbors=5, derivative_indices=[0], radius=None, regularize_lstsq=False)"
    assert str(inspect.signature(neuraloperator_amd.get_non_uniform_fd_weights)) == ref_sig
    assert str(inspect.signature(neuraloperator_amd.NonUniformFD.__init__)) == ref_sig.replace("(points", "(self, points")
    assert str(inspect.signature(neuraloperator_amd.non_uniform_fd)) == ref_sig.replace("(points,", "(points, values,")
    p = torch.rand(7, 2, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    for want, k in ((1, 3), (2, 3), (5, 5), (7, 7), (50, 7)):                # k = min(max(num_neighbors, 3), N)
        idx, w = D.get_non_uniform_fd_weights(p, num_neighbors=want, derivative_indices=[1, 0])
        assert idx.shape == (7, k) and w.shape == (7, 2, k) and idx.dtype == torch.int64
        assert D.NonUniformFD(p, num_neighbors=want).k == k
    with pytest.raises(ValueError, match="route must be one of"):
        with D.route("hip"):
            pass


def test_ineligible_calls_stay_on_torch_and_the_engine_route_refuses_them():
    gen = torch.Generator().manual_seed(1)
    p32 = torch.rand(40, 2, generator=gen)
    v32 = torch.rand(40, generator=gen)
    with engine_on_emulation():                              # CPU tensors count as device tensors in here
        assert D.on_engine(p32, v32)
        kinds = {
            "float64 points": dict(points=p32.double(), values=v32.double()),
            "float64 values": dict(points=p32, values=v32.double()),
            "points (N,)": dict(points=p32[:, 0], values=v32),
            "d = 4": dict(points=torch.rand(40, 4, generator=gen), values=v32),
            "k > 32": dict(points=p32, values=v32, num_neighbors=33),
            "k < d + 1": dict(points=torch.rand(3, 3, generator=gen), values=v32[:3], num_neighbors=3),
            "derivative index outside [0, d)": dict(points=p32, values=v32, derivative_indices=[2]),
            "nine derivative indices": dict(points=p32, values=v32, derivative_indices=[0] * 9),
            "radius with d = 3": dict(points=torch.rand(40, 3, generator=gen), values=v32, radius=0.4),
            "points need a gradient": dict(points=p32.clone().requires_grad_(), values=v32),
        }
        for kind, kw in kinds.items():
            assert not D.on_engine(**kw), kind
            for call in (D.non_uniform_fd, lambda points, values, **k: D.NonUniformFD(points, **k)(values)):
                with D.route("engine"), pytest.raises(ValueError, match="not eligible"):
                    call(**kw)
        with D.route("torch"):
            assert not D.on_engine(p32, v32)
            fd = D.NonUniformFD(p32)
            assert fd._stencil is None and not fd.on_engine(v32)
        fd = D.NonUniformFD(p32)
        assert fd.on_engine(v32) and not fd.on_engine(v32.double()) and not fd.on_engine(v32[:5])
        with D.route("engine"), pytest.raises(ValueError, match="not eligible"):
            fd(v32.double())
        with pytest.raises(ValueError, match=r"\(\.\.\., 40\)"):
            fd(v32[:5])
    assert not D.on_engine(p32, v32)                         # CPU tensors outside the emulation
    # gradients with respect to the points stay on the torch route and exist
    pg = p32.double().requires_grad_()
    D.non_uniform_fd(pg, v32.double(), num_neighbors=6).sum().backward()
    assert pg.grad is not None and bool(torch.isfinite(pg.grad).all())


def test_tie_share_of_every_knn_case_from_the_float64_sort_alone():
    """no engine: the share of queries whose k-th and (k + 1)-th finite distances lie within the band stays below the
    cap on every KNN_CASES entry, so the seeds leave the comparisons their force; and the table names the edges"""
    for name, cfg in nr.KNN_CASES.items():
        assert nr.knn_tie_share(cfg) <= nr.MAX_TIE_SHARE == 0.05, name
    K = nr.KNN_CASES.values()
    assert {1, 7, 8, 9, 31, 32, 33, 65} <= {c["m"] for c in K if (c["n"], c["d"], c["k"]) == (200, 2, 5)}
    for k in (32, 3):
        for d in (1, 3):
            assert {63, 64, 65, 127, 128, 129} <= {c["n"] for c in K if (c["k"], c["d"]) == (k, d)}, (k, d)
    assert any(c["kind"] == "descending" and (c["n"], c["k"]) == (129, 32) for c in K)
    assert any((c["n"], c["k"]) == (33, 32) for c in K) and {"nan_tenth", "few_finite", "nan_query"} <= {c["kind"] for c in K}
    assert (nr.QPW, nr.QPB, nr.LANES) == (8, 32, 64)
