"""CPU tier: the project's own piecewise linear filter basis (neuraloperator_amd/filter_basis.py) against ITS DEFINITION:
the value is 1 at each node and 0 at the neighbouring nodes, no entry lies beyond r_cutoff, the hats sum to 1 inside the
cutoff, the index layout is (basis, out, in) in argwhere order.  Nothing here compares the basis with torch_harmonics:
that package is not available to this project's tests, and the basis has not been checked against it."""
import math

import pytest
import torch

from neuraloperator_amd.filter_basis import PiecewiseLinearFilterBasis, basis_class

R = 0.3


def _dense(basis, r, phi):
    idx, vals = basis.compute_support_vals(r, phi, r_cutoff=R)
    out = torch.zeros(basis.kernel_size, *r.shape, dtype=vals.dtype)
    out[idx[:, 0], idx[:, 1], idx[:, 2]] = vals
    return out, idx, vals


@pytest.mark.parametrize("shape", [[2, 4], [3, 3], [3, 4], [4, 1], [2, 2]])
def test_one_at_its_node_zero_at_the_neighbouring_nodes(shape):
    nr, nphi = shape
    b = PiecewiseLinearFilterBasis(shape)
    assert b.kernel_size == (nr - 1) * nphi + 1
    dr, dphi = R / (nr - 1), 2 * math.pi / nphi
    nodes = [(0.0, 0.0)] + [(ir * dr, ip * dphi) for ir in range(1, nr) for ip in range(nphi)]
    r = torch.tensor([[n[0] for n in nodes]], dtype=torch.float64)
    phi = torch.tensor([[n[1] for n in nodes]], dtype=torch.float64)
    dense, _, _ = _dense(b, r, phi)
    got = dense[:, 0, :]                                     # [basis, node]
    for k in range(b.kernel_size):
        assert abs(float(got[k, k]) - 1.0) < 1e-12, k
        for j in range(b.kernel_size):
            if j != k:
                assert abs(float(got[k, j])) < 1e-12, (k, j)


def test_basis_0_is_the_radial_hat_and_the_angle_wraps():
    b = PiecewiseLinearFilterBasis([3, 4])
    dr = R / 2
    r = torch.tensor([[0.0, dr / 4, dr / 2, dr, 1.5 * dr]], dtype=torch.float64)
    phi = torch.zeros_like(r)
    dense, _, _ = _dense(b, r, phi)
    assert torch.allclose(dense[0, 0], torch.tensor([1.0, 0.75, 0.5, 0.0, 0.0], dtype=torch.float64), atol=1e-12)
    # basis 1: ring 1, angle 0 -- the same value just below 2 pi as just above 0
    eps = 0.1
    r2 = torch.full((1, 2), dr, dtype=torch.float64)
    phi2 = torch.tensor([[eps, 2 * math.pi - eps]], dtype=torch.float64)
    d2, _, _ = _dense(b, r2, phi2)
    want = 1.0 - eps / (2 * math.pi / 4)
    assert abs(float(d2[1, 0, 0]) - want) < 1e-12 and abs(float(d2[1, 0, 1]) - want) < 1e-12
    # halfway between ring 1 and ring 2, halfway between angle nodes 1 and 2: a quarter each for the four neighbours
    d3, _, _ = _dense(b, torch.tensor([[1.5 * dr]], dtype=torch.float64),
                      torch.tensor([[1.5 * 2 * math.pi / 4]], dtype=torch.float64))
    near = {1 + 1, 1 + 2, 1 + 4 + 1, 1 + 4 + 2}
    for k in range(b.kernel_size):
        assert abs(float(d3[k, 0, 0]) - (0.25 if k in near else 0.0)) < 1e-12, k


@pytest.mark.parametrize("shape", [[2, 4], [3, 3], [3, 4], [5, 2]])
def test_no_entry_beyond_the_cutoff_and_the_hats_sum_to_one_inside(shape):
    gen = torch.Generator().manual_seed(1)
    r = torch.rand(3, 200, generator=gen, dtype=torch.float64) * (1.4 * R)
    phi = torch.rand(3, 200, generator=gen, dtype=torch.float64) * 2 * math.pi
    b = PiecewiseLinearFilterBasis(shape)
    dense, idx, vals = _dense(b, r, phi)
    assert bool((r[idx[:, 1], idx[:, 2]] <= R).all()) and bool((vals > 0).all())
    inside = r <= R
    assert inside.any() and (~inside).any()
    total = dense.sum(0)
    assert torch.allclose(total[inside], torch.ones_like(total[inside]), atol=1e-12)
    assert not total[~inside].any()
    # the radial hats alone: basis 0 plus, per ring, the sum over its angular nodes
    nr, nphi = shape
    rings = [dense[0]] + [dense[1 + i * nphi:1 + (i + 1) * nphi].sum(0) for i in range(nr - 1)]
    dr = R / (nr - 1)
    for i, ring in enumerate(rings):
        want = (1.0 - (r - i * dr).abs() / dr).clamp(min=0.0) * inside
        assert torch.allclose(ring, want, atol=1e-12), i


def test_index_layout():
    b = PiecewiseLinearFilterBasis([2, 4])
    gen = torch.Generator().manual_seed(2)
    r = torch.rand(4, 9, generator=gen) * (1.2 * R)
    phi = torch.rand(4, 9, generator=gen) * 2 * math.pi
    idx, vals = b.compute_support_vals(r, phi, r_cutoff=R)
    assert idx.dtype == torch.int64 and idx.dim() == 2 and idx.shape[1] == 3 and vals.shape == (idx.shape[0],)
    assert vals.dtype == r.dtype
    assert int(idx[:, 0].max()) < b.kernel_size and int(idx[:, 1].max()) < 4 and int(idx[:, 2].max()) < 9
    flat = (idx[:, 0] * 4 + idx[:, 1]) * 9 + idx[:, 2]
    assert bool((flat[1:] > flat[:-1]).all())                # argwhere order, no duplicates
    assert PiecewiseLinearFilterBasis(3).kernel_shape == [3, 3]


def test_names_without_the_real_package():
    try:
        import torch_harmonics.filter_basis  # noqa: F401
        return                                               # the real package is there: the layers use its classes
    except ImportError:
        pass
    assert basis_class("piecewise_linear") is PiecewiseLinearFilterBasis
    for name in ("morlet", "zernike"):
        with pytest.raises(NotImplementedError, match="torch_harmonics"):
            basis_class(name)
