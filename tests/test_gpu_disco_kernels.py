"""GPU tier: the equidistant discrete-continuous convolution kernels (sc_kernels_disco.h) at their tile, stride, chunk
and route edges on an MI355X, driven through the C-ABI with free-standing descriptors (disco_reference.run_descriptor:
a random basis buffer, any support / stride / padding the entry points accept) against the float64 helper on the host.
The cases are disco_reference.KERNEL_CASES:
  a  every row stride one row past its tile (tr = 16, 8, 4, 4) and one column past DC_TC, mixed strides
  b  the widest (267 columns) and the tallest (30 rows) LDS tile filled with data: support 15 x 15, stride 4 and 1
  c  padding 0 and support - 1, an even and a 1 x 9 support, strides 1 and 3
  d  the transposed form at strides (3, 4) and (4, 3), both ends of output_padding, negative floordiv arguments
  e  channels of a group around DC_OCB in both directions, groups, depthwise
  f  the weight gradient: pw on both sides of its two reduction batches with a stride, one chunk, 32 chunks over 33
     units (15 empty), 1 and 40 basis functions, the bias gradient at 255 / 256 / 257 points
  g  the matrix-core body at the nine channel pairs, plain and transposed, with and without bias; 65 units, 64 chunks
  h  the descriptor list of the emulation tier (disco_reference.DESC_CASES)
Every case runs forward, data, weight and bias gradient and is held to two bars: the whole-tensor rel-L2 of the project
(1e-5) and, per element, |got - want| <= gamma_N A with A and N from disco_reference.abs_bounds (derived from the
kernel source, not measured)."""
import pytest
import torch

import disco_reference as dr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("out", "grad:x", "grad:weight", "grad:bias")
ALL_CASES = {**dr.KERNEL_CASES, **{"h_" + k: v for k, v in dr.DESC_CASES.items()}}


def _lib():
    from neuraloperator_amd import _lib
    return _lib.get_lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run(cfg, *tensors, **kw):
    return dr.run_descriptor(_lib(), cfg, *tensors, device=DEV, stream=_stream(), **kw)


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_kernel_edges_against_the_float64_helper(name):
    cfg = ALL_CASES[name]
    x, w, psi, b, g = dr.desc_inputs(cfg, 91)
    assert _lib().disco_path(dr.desc_of(cfg, g.shape[2:])) == cfg["route"]
    got = [t.numpy() for t in _run(cfg, x, w, psi, b, g)]
    want = [t.numpy() for t in dr.desc_want(cfg, x, w, psi, b, g)]
    bounds, ns = dr.abs_bounds(cfg, x, w, psi, b, g)
    errs = [dr.rel_l2(a, t) for a, t in zip(got, want)]
    ratios = [dr.worst_ratio(a, t, A.numpy(), n) for a, t, A, n in zip(got, want, bounds, ns)]
    print(name, "rel_l2", " ".join(f"{e:.1e}" for e in errs), "worst |err| / (gamma_N A)",
          " ".join(f"{k}={r:.3f} (N={n})" for k, r, n in zip(NAMES, ratios, ns)))
    assert max(errs) <= 1e-5, errs
    for k, r in zip(NAMES, ratios):
        assert r <= 1.0, (k, r)


def test_the_chunk_plans_the_cases_are_cut_for():
    """(units, chunks, per_chunk) as dc_plan cuts them: what two cases of group f and the last of group g are about"""
    def plan(name):
        cfg = dr.KERNEL_CASES[name]
        shape = dr.out_shape_of((cfg["batch"], cfg["c_in"], *cfg["in_shape"]), cfg["c_out"], (cfg["basis"], *cfg["support"]),
                                cfg["stride"], cfg["padding"], cfg["opad"], cfg["transposed"])
        return dr.wgrad_plan(cfg, shape[2:])[:3]
    assert plan("f_one_chunk_33_31") == (1, 1, 1)
    assert plan("f_33_units_32_chunks") == (33, 32, 2)                 # chunk 16 holds one unit, 17 .. 31 none
    assert plan("g_mfma_32_32_49x129_65_units") == (65, 64, 2)         # 33 chunks carry data


def test_the_bias_gradient_alone_needs_no_workspace():
    cfg = dr.KERNEL_CASES["f_gbias_257_points"]
    x, w, psi, b, g = dr.desc_inputs(cfg, 93)
    gd = g.to(DEV)
    gb = torch.full((cfg["c_out"],), float("nan"), device=DEV)
    _lib().disco_backward(dr.desc_of(cfg, g.shape[2:]), 0, 0, 0, gd.data_ptr(), 0, 0, gb.data_ptr(), 0, 0, _stream())
    joint = _run(cfg, x, w, psi, b, g)
    assert torch.equal(gb.cpu(), joint[3])
    want = g.double().sum(dim=(0, 2, 3)).numpy()
    assert dr.rel_l2(gb.cpu().numpy(), want) <= 1e-5
    n = dr.roundings(cfg, tuple(g.shape[2:]))[3]
    assert dr.worst_ratio(gb.cpu().numpy(), want, g.double().abs().sum(dim=(0, 2, 3)).numpy(), n) <= 1.0


@pytest.mark.parametrize("name", ["a_stride_3x4", "d_transpose_4x3_opad32_groups2", "g_mfma_64_32",
                                  "g_mfma_32_32_49x129_65_units"])
def test_one_gradient_alone_and_a_repeat_give_the_same_bits(name):
    cfg = dr.KERNEL_CASES[name]
    args = dr.desc_inputs(cfg, 92)
    a, c = _run(cfg, *args), _run(cfg, *args)
    assert all(torch.equal(u, v) for u, v in zip(a, c))
    for i in range(3):
        want = tuple(j == i for j in range(3))
        one = _run(cfg, *args, want=want)
        assert torch.equal(one[1 + i], a[1 + i]) and sum(t is not None for t in one[1:]) == 1
