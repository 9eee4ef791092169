"""GPU tier: the point-cloud discrete-continuous convolution kernels (sc_kernels_disco_sparse.h) at their round, tile,
slice and route edges on an MI355X, driven through the C-ABI with free-standing descriptors over a random Psi
(disco_sparse_reference.run_descriptor) against the float64 helper on the host.  The cases are
disco_sparse_reference.KERNEL_DESC_CASES:
  a  the 128-column rounds of k_dsp_contract: a group that straddles a round, three rounds, both directions, depthwise
  b  the tiles of k_dsp_wgrad: output channels around DSP_WG_OC, (k, c) columns around DSP_WG_J, rows around DSP_WG_R
  c  the cap of 64 slices on both routes, an odd per_slice on the matrix cores
  d  the matrix-core route at the nine channel pairs, rows around DSPM_ROWS, 1 and 3 basis functions, a ragged last trip
  e  one gradient alone, bit-equal to the joint run, on both routes
Every case runs forward, data, weight and bias gradient and is held to two bars: the whole-tensor rel-L2 of the project
(1e-5) and, per element, |got - want| <= gamma_N A with A and N from disco_sparse_reference.abs_bounds (derived from the
kernel source, not measured).  Only in-range CSR indices reach the device."""
import pytest
import torch

import disco_sparse_reference as ds

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("out", "grad:x", "grad:weight", "grad:bias")


def _lib():
    from neuraloperator_amd import _lib
    return _lib.get_lib()


def _run(cfg, *tensors, **kw):
    return ds.run_descriptor(_lib(), cfg, *tensors, device=DEV, stream=torch.cuda.current_stream().cuda_stream, **kw)


@pytest.mark.parametrize("name", sorted(ds.KERNEL_DESC_CASES))
def test_kernel_edges_against_the_float64_helper(name):
    cfg = ds.KERNEL_DESC_CASES[name]
    psi, keep, x, w, q, b, g = ds.desc_inputs(cfg, 91)
    assert int(keep.sum(dim=2).max()) <= 4 or cfg["n_out"] < 1000        # the long clouds: 0 to 4 entries to a row
    got = _run(cfg, psi, keep, x, w, q, b, g)                            # asserts the route
    want = ds.sparse_disco_with_grads(x, w, b, psi.double(), q, g, cfg["groups"])
    bounds, ns = ds.abs_bounds(cfg, psi, keep, x, w, q, b, g)
    errs = [ds.rel_l2(a.numpy(), t.numpy()) if float(t.abs().max()) > 0 else float(a.abs().max())
            for a, t in zip(got[:4], want)]
    ratios = [ds.worst_ratio(a.numpy(), t.numpy(), A.numpy(), n) for a, t, A, n in zip(got[:4], want, bounds, ns)]
    print(name, "rel_l2", " ".join(f"{e:.1e}" for e in errs), "worst |err| / (gamma_N A)",
          " ".join(f"{k}={r:.3f} (N={n})" for k, r, n in zip(NAMES, ratios, ns)))
    assert max(errs) <= 1e-5, errs
    for k, r in zip(NAMES, ratios):
        assert r <= 1.0, (k, r)


def test_the_slice_plans_the_cases_are_cut_for():
    """(slices, per_slice) as dsp_plan cuts the rows"""
    plan = {k: ds.wgrad_slices(v) for k, v in ds.KERNEL_DESC_CASES.items()}
    assert plan["c_slice_cap_rows_16130"] == (64, 253)
    assert plan["c_slice_cap_mfma_rows_16400_per_slice_257"] == (64, 257)
    assert plan["d_mfma_32_32_rows129"] == (1, 129)                      # 129 = 16 * 8 + 1: a last trip of one row


@pytest.mark.parametrize("name", ["a_data_gradient_og96_straddles", "d_mfma_64_32_rows129"])
def test_one_gradient_alone_and_a_repeat_give_the_same_bits(name):
    cfg = ds.KERNEL_DESC_CASES[name]
    args = ds.desc_inputs(cfg, 92)
    a, c = _run(cfg, *args), _run(cfg, *args)
    assert all(torch.equal(u, v) for u, v in zip(a, c))
    for i in range(3):                                                   # gx / gw / gbias alone in turn
        want = tuple(j == i for j in range(3))
        one = _run(cfg, *args, want=want)
        assert torch.equal(one[1 + i], a[1 + i]) and sum(t is not None for t in one[1:4]) == 1
