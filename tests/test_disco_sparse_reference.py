"""CPU tier: DiscreteContinuousConv2d / DiscreteContinuousConvTranspose2d on point clouds against fixtures recorded from
the verbatim reference classes (tests/record_disco_sparse.py, tests/golden/dsparse_*.npz), the engine in host emulation:
attributes, the entries of Psi and their order, the values of Psi, out and every gradient to 1e-5 rel-L2 of the float64
record, the constructor's errors, the state dict, the torch fallback on CPU tensors, and the construction of Psi in row
blocks (bit-identical whatever the block, no n_out x n_in tensor)."""
import numpy as np
import pytest
import torch

import disco_sparse_reference as ds
from conftest import load_golden
from emu_engine import engine_on_emulation

NAMES = sorted(ds.CASES)


@pytest.fixture
def emu():                                                   # per test: the fallback tests run without it
    with engine_on_emulation() as lib:
        yield lib


@pytest.fixture(scope="module")
def built():
    """every case's record and the project's layer built from the record's own grids, once"""
    out = {}
    for name in NAMES:
        cfg, rec = ds.CASES[name], load_golden("dsparse_" + name)
        m = ds.own_class(cfg["transposed"])(grid_in=torch.from_numpy(rec["grid_in"]),
                                            grid_out=torch.from_numpy(rec["grid_out"]),
                                            quadrature_weights=torch.from_numpy(rec["q"]), **cfg["kwargs"])
        out[name] = (cfg, rec, m)
    return out


def _normalised(cfg):
    k0, k1 = (cfg["kwargs"]["kernel_shape"],) * 2 if isinstance(cfg["kwargs"]["kernel_shape"], int) else \
        cfg["kwargs"]["kernel_shape"]
    return (k0 // 2) * k1 + k0 % 2


@pytest.mark.parametrize("name", NAMES)
def test_attributes_and_entries(built, name):
    cfg, rec, m = built[name]
    grid_in, grid_out, q = ds.case_grids(cfg, int(rec["seed"]))          # the record is what the case table says
    assert np.array_equal(grid_in.numpy(), rec["grid_in"]) and np.array_equal(q.numpy(), rec["q"])
    assert np.array_equal(grid_out.numpy(), rec["grid_out"])
    assert list(m.kernel_shape) == [int(v) for v in rec["kernel_shape"]]
    for a in ds.NUMERIC_ATTRS:
        assert getattr(m, a) == rec["attr:" + a], a
    assert m.psi_idx.dtype == torch.int64 and tuple(m.psi_idx.shape) == tuple(rec["psi_idx"].shape)
    assert np.array_equal(m.psi_idx.numpy(), rec["psi_idx"].astype(np.int64))          # the same set in the same order
    assert m.psi_vals.dtype == (torch.float64 if cfg["float64"] else torch.float32)
    assert [k for k, _ in m.named_buffers()] == ["quadrature_weights", "psi_idx", "psi_vals", "csr_splits", "csr_cols",
                                                 "csr_vals", "csr_t_splits", "csr_t_cols", "csr_t_vals"]
    psi = m.get_local_filter_matrix()
    assert psi.is_sparse and tuple(psi.shape) == (m.kernel_size * m.n_out, m.n_in)
    if cfg["lonely"]:                                                    # no entry at the far output point
        assert not bool(((m.psi_idx[0] % m.n_out) == ds.LONELY).any())


@pytest.mark.parametrize("name", NAMES)
def test_psi_values(built, name):
    cfg, rec, m = built[name]
    k = rec["psi_idx"][0].astype(np.int64) // m.n_out
    norm = k < _normalised(cfg)
    got, want = m.psi_vals.numpy(), rec["psi_vals"]
    assert np.array_equal(got[~norm], want[~norm]) and (~norm).any() and norm.any()
    deg_max = int(np.bincount(rec["psi_idx"][0].astype(np.int64)[norm]).max())       # row = (basis, output point)
    rel = np.abs(got[norm].astype(np.float64) - want[norm]) / np.abs(want[norm])
    bound = (deg_max + 2) * 2.0 ** -24
    print(name, f"deg_max {deg_max} worst {rel.max():.2e} bound {bound:.2e}")
    assert rel.max() <= bound


def test_engine_forms_of_psi(built):
    """the two CSR forms hold Psi's entries: rows (o, k) with ascending input points, rows i with ascending (o, k)"""
    for name in ("default", "transpose_r0.2_3x4"):
        cfg, rec, m = built[name]
        K, dense = m.kernel_size, ds.layer_psi(m)
        for splits, cols, vals, by_input in ((m.csr_splits, m.csr_cols, m.csr_vals, False),
                                             (m.csr_t_splits, m.csr_t_cols, m.csr_t_vals, True)):
            assert splits.dtype == torch.int32 and cols.dtype == torch.int32 and vals.dtype == torch.float32
            rows = m.n_in if by_input else m.n_out * K
            assert splits.numel() == rows + 1 and int(splits[0]) == 0 and int(splits[-1]) == vals.numel()
            r = torch.repeat_interleave(torch.arange(rows), (splits[1:] - splits[:-1]).long())
            key = r * (m.n_out * K if by_input else m.n_in) + cols.long()
            assert bool((key[1:] > key[:-1]).all())                      # ascending, duplicate-free
            ok, i = (cols.long(), r) if by_input else (r, cols.long())
            rebuilt = torch.zeros_like(dense)
            rebuilt[ok % K, ok // K, i] = vals.double()
            assert torch.equal(rebuilt, dense.float().double())


def _errors(got, rec):
    out, gx, gw, gb = got
    errs = {"out": ds.rel_l2(out, rec["out"]), "grad:x": ds.rel_l2(gx, rec["grad:x"]),
            "grad:weight": ds.rel_l2(gw, rec["grad:weight"])}
    if gb is not None:
        errs["grad:bias"] = ds.rel_l2(gb, rec["grad:bias"])
    return errs


@pytest.mark.parametrize("name", NAMES)
def test_layer_on_the_engine_matches_the_record(emu, built, name):
    cfg, rec, m = built[name]
    x = torch.from_numpy(rec["x"])
    assert m.on_engine(x) == (not cfg["float64"])            # float64 buffers: the torch formula
    errs = _errors(ds.run_module(m, rec, "cpu"), rec)
    print(name, " ".join(f"{k}={e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= 1e-5, (k, e)
    if cfg["lonely"]:
        out = m(x).detach()
        assert torch.equal(out[:, :, ds.LONELY], m.bias.detach().expand(out.shape[0], -1))


@pytest.mark.parametrize("name", NAMES)
def test_torch_fallback_on_cpu_tensors(built, name):
    cfg, rec, m = built[name]
    assert not m.on_engine(torch.from_numpy(rec["x"]))
    errs = _errors(ds.run_module(m, rec, "cpu"), rec)
    for k, e in errs.items():
        assert e <= 1e-5, (k, e)


def test_fallback_in_float64_and_the_helper_agree_with_the_record(built):
    cfg, rec, m = built["groups2"]
    want = ds.sparse_disco_with_grads(torch.from_numpy(rec["x"]), torch.from_numpy(rec["weight"]),
                                      torch.from_numpy(rec["bias"]), ds.dense_psi(rec["psi_idx"], rec["psi_vals"],
                                                                                  m.kernel_size, m.n_out, m.n_in),
                                      torch.from_numpy(rec["q"]), torch.from_numpy(rec["g"]), m.groups)
    for a, k in zip(want, ("out", "grad:x", "grad:weight", "grad:bias")):
        assert ds.rel_l2(a.numpy(), rec[k]) <= 1e-12, k
    m64 = ds.build_own(cfg, int(rec["seed"])).double()
    errs = _errors(ds.run_module(m64, rec, "cpu"), rec)
    assert max(errs.values()) <= 1e-5, errs


def test_state_dict_loads_a_reference_shaped_one_strictly(built):
    for name in ("default", "no_bias", "transpose_grouped"):
        cfg, rec, m = built[name]
        assert list(m.state_dict()) == [str(k) for k in rec["state_keys"]]
        state = {"weight": torch.from_numpy(rec["weight"])}
        if "bias" in rec:
            state["bias"] = torch.from_numpy(rec["bias"])
        fresh = ds.build_own(cfg, int(rec["seed"]))
        assert fresh.load_state_dict(state, strict=True).missing_keys == []
        assert torch.equal(fresh.weight.detach(), state["weight"])


def test_initial_weight_scale_and_default_cutoffs():
    import math
    import neuraloperator_amd as na
    from neuraloperator_amd import discrete_continuous_convolution as dcc
    g = torch.Generator().manual_seed(3)
    gi, go, q = torch.rand(2, 60, generator=g), torch.rand(2, 40, generator=g), torch.ones(60) / 60
    torch.manual_seed(11)
    m = na.DiscreteContinuousConv2d(64, 64, gi, go, [2, 4], quadrature_weights=q, groups=4)
    assert tuple(m.weight.shape) == (64, 16, 5) and m.groupsize == 16
    assert abs(float(m.weight.detach().std()) - math.sqrt(1.0 / 16)) < 0.02 and float(m.bias.detach().abs().sum()) == 0.0
    # the default cut-off is 2 / (sqrt(n_out) - 1), and 2 / (sqrt(n_in) - 1) for the transpose: the same Psi as with it given
    for cls, n in ((na.DiscreteContinuousConv2d, 40), (na.DiscreteContinuousConvTranspose2d, 60)):
        a = cls(2, 2, gi, go, [2, 4], quadrature_weights=q)
        b = cls(2, 2, gi, go, [2, 4], quadrature_weights=q, radius_cutoff=2 / float(math.sqrt(n) - 1))
        c = cls(2, 2, gi, go, [2, 4], quadrature_weights=q, radius_cutoff=1.1 * 2 / float(math.sqrt(n) - 1))
        assert torch.equal(a.psi_idx, b.psi_idx) and torch.equal(a.psi_vals, b.psi_vals)
        assert c.psi_vals.numel() > a.psi_vals.numel()
    assert dcc.PSI_ROW_BLOCK <= 1024


def test_constructor_errors_match_the_reference():
    import neuraloperator_amd as na
    gi, go, q = torch.rand(2, 20), torch.rand(2, 10), torch.ones(20) / 20
    classes = [na.DiscreteContinuousConv2d, na.DiscreteContinuousConvTranspose2d]
    if ds.reference_available():                             # the verbatim classes raise the same
        classes += [ds.reference_class(False), ds.reference_class(True)]
    for cls in classes:
        with pytest.raises(ValueError, match="input channels has to be an integer multiple"):
            cls(3, 4, gi, go, [2, 4], quadrature_weights=q, groups=2)
        with pytest.raises(ValueError, match="output channels has to be an integer multiple"):
            cls(4, 3, gi, go, [2, 4], quadrature_weights=q, groups=2)
        with pytest.raises(ValueError, match="radius_cutoff has to be positive"):
            cls(4, 4, gi, go, [2, 4], quadrature_weights=q, radius_cutoff=0.0)
        with pytest.raises(AssertionError):
            cls(4, 4, gi, go, [2, 4])                        # a tensor grid needs tensor quadrature weights
        with pytest.raises(AssertionError):
            cls(4, 4, gi, go, [2, 4], quadrature_weights=q, periodic=True)
        with pytest.raises(ValueError, match="Unknown grid input type"):
            cls(4, 4, [0.0, 1.0], go, [2, 4], quadrature_weights=q)
        with pytest.raises(ValueError, match="Unknown grid output type"):
            cls(4, 4, gi, None, [2, 4], quadrature_weights=q)
        with pytest.raises(AssertionError):
            cls(4, 4, gi.reshape(-1), go, [2, 4], quadrature_weights=q)
        with pytest.raises(AssertionError):
            cls(4, 4, torch.rand(3, 20), go, [2, 4], quadrature_weights=q)
        with pytest.raises(AssertionError):
            cls(4, 4, gi, go, [2, 4], quadrature_weights=q.reshape(1, -1))
        with pytest.raises(AssertionError):
            cls(4, 4, "equidistant", go, [2, 4])             # a string grid needs n_in
    try:
        import torch_harmonics  # noqa: F401
    except ImportError:
        for cls in classes[:2]:
            with pytest.raises(NotImplementedError, match="torch_harmonics"):
                cls(4, 4, "equidistant", go, [2, 4], n_in=(4, 5))
            with pytest.raises(NotImplementedError, match="torch_harmonics"):
                cls(4, 4, gi, "equidistant", [2, 4], n_out=(4, 5), quadrature_weights=q)


def _buffers(m):
    return {k: v.clone() for k, v in m.named_buffers()}


def test_row_blocks_give_the_same_bits(monkeypatch):
    from neuraloperator_amd import discrete_continuous_convolution as dcc
    got = {}
    for name in ("kernel_shape_3x4_r0.2", "transpose_default"):
        cfg = ds.CASES[name]
        for block in (7, 10 ** 6):
            monkeypatch.setattr(dcc, "PSI_ROW_BLOCK", block)
            got[block] = _buffers(ds.build_own(cfg, 41))
        assert list(got[7]) == list(got[10 ** 6])
        for k in got[7]:
            assert torch.equal(got[7][k], got[10 ** 6][k]), (name, k)


def test_arctan2_does_not_depend_on_the_position():
    """the same pairs at the front, in the middle and at the very end of arrays of odd lengths give the same bits (torch's
    own arctan2 gives its array tails to another routine: the assumption _arctan2 documents)"""
    from neuraloperator_amd.discrete_continuous_convolution import _arctan2
    g = torch.Generator().manual_seed(7)
    for dtype in (torch.float32, torch.float64):
        y, x = (torch.rand(1000, generator=g, dtype=dtype) - 0.5 for _ in range(2))
        want = _arctan2(y[:960], x[:960])                    # whole vectors only
        assert torch.equal(want, torch.arctan2(y[:960], x[:960]))
        for n, shift in ((977, 17), (40000, 39040), (16384 + 960 + 3, 16384 + 3)):
            yy, xx = torch.ones(n, dtype=dtype), torch.ones(n, dtype=dtype)
            yy[shift:shift + 960], xx[shift:shift + 960] = y[:960], x[:960]
            assert torch.equal(_arctan2(yy, xx)[shift:shift + 960], want), (dtype, n, shift)
        assert torch.equal(_arctan2(y.reshape(8, 125), x.reshape(8, 125)).reshape(-1)[:960], want)


def test_no_tensor_of_n_out_times_n_in_elements(monkeypatch):
    """3000 x 3000 points in row blocks of 64: the largest array the basis is given has 64 x 3000 elements, and the
    buffers are those of the default block"""
    import neuraloperator_amd as na
    from neuraloperator_amd import discrete_continuous_convolution as dcc
    from neuraloperator_amd import filter_basis
    g = torch.Generator().manual_seed(5)
    n = 3000
    gi, go, q = torch.rand(2, n, generator=g), torch.rand(2, n, generator=g), torch.rand(n, generator=g) / n
    seen = []
    basis = filter_basis.basis_class("piecewise_linear")
    inner = basis.compute_support_vals

    def spy(self, r, phi, r_cutoff):
        seen.append(max(r.numel(), phi.numel()))
        return inner(self, r, phi, r_cutoff)

    monkeypatch.setattr(basis, "compute_support_vals", spy)
    want = _buffers(na.DiscreteContinuousConv2d(2, 2, gi, go, [2, 4], quadrature_weights=q))
    assert max(seen) <= dcc.PSI_ROW_BLOCK * n < n * n
    del seen[:]
    monkeypatch.setattr(dcc, "PSI_ROW_BLOCK", 64)
    got = _buffers(na.DiscreteContinuousConv2d(2, 2, gi, go, [2, 4], quadrature_weights=q))
    assert len(seen) == -(-n // 64) and max(seen) == 64 * n
    for k in want:
        assert torch.equal(got[k], want[k]), k
