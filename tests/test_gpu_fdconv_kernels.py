"""GPU tier: the finite-difference convolution kernels (sc_kernels_fdconv.h) at their tile, chunk and route edges on an
MI355X, driven through the C-ABI with free-standing descriptors (fdconv_reference.run_descriptor) against the float64
helper on the host.  The cases are fdconv_reference.KERNEL_CASES:
  a  general route one past FD_TR x FD_TC, k = 3 / 5 / 7 in the four modes; k = 7 at (33, 130), replicate and reflect
  b  replicate / reflect data gradient whose padded extents d + 2 r cross a tile while d does not
  c  the smallest legal extents: reflect n = r + 1, periodic n = r (taps alias), periodic n = 1
  d  three axes, planes outside the field
  e  output channels of a group around FD_OCB, groups, depthwise
  f  the chunks of the weight gradient: one chunk, 32 chunks over 33 units (15 empty), 11 over 11
  g  the matrix-core body at the nine channel pairs, its smallest tiles, 65 units over 64 chunks
Every case runs forward, data gradient and weight gradient and is held to two bars: the whole-tensor rel-L2 of the
project (1e-5) and, per element, |got - want| <= gamma_N A with A and N from fdconv_reference.abs_bounds (derived from
the kernel source, not measured).  Where A is 0 -- the centre tap's gradient -- the value must be exactly 0."""
import pytest
import torch

import fdconv_reference as fr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = ("out", "grad:x", "grad:weight")


def _lib():
    from neuraloperator_amd import _lib
    return _lib.get_lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run(cfg, x, w, g, h, **kw):
    return fr.run_descriptor(_lib(), cfg, x, w, g, h, device=DEV, stream=_stream(), **kw)


@pytest.mark.parametrize("name", sorted(fr.KERNEL_CASES))
def test_kernel_edges_against_the_float64_helper(name):
    cfg = fr.KERNEL_CASES[name]
    x, w, g = fr.case_inputs(cfg, 91)
    h = fr.grid_width_of(cfg)
    assert _lib().fdconv_path(fr.desc_of(cfg, h)) == cfg["route"]
    got = [t.numpy() for t in _run(cfg, x, w, g, h)]
    want = [t.numpy() for t in fr.fdconv_with_grads(x, w, g, h, cfg["groups"], cfg["padding"])]
    bounds, ns = fr.abs_bounds(cfg, x, w, g, h)
    ratios = [fr.worst_ratio(a, b, A, n) for a, b, A, n in zip(got, want, bounds, ns)]
    errs = [fr.rel_l2(a, b, z) for a, b, z in zip(got, want, fr.magnitudes(x, w, g, h, cfg["groups"], cfg["padding"]))]
    print(name, "rel_l2", " ".join(f"{e:.1e}" for e in errs), "worst |err| / (gamma_N A)",
          " ".join(f"{k}={r:.3f} (N={n})" for k, r, n in zip(NAMES, ratios, ns)))
    fr.check_against(cfg, got, want, (1e-5, 1e-5, 1e-5), fr.magnitudes(x, w, g, h, cfg["groups"], cfg["padding"]))
    for k, r in zip(NAMES, ratios):
        assert r <= 1.0, (k, r)


def test_the_chunk_plans_the_cases_are_cut_for():
    """(units, chunks, per_chunk) as fd_plan cuts them: what group f and the last case of group g are about"""
    plan = {k: fr.wgrad_plan(fr.KERNEL_CASES[k])[:3] for k in fr.KERNEL_CASES}
    assert plan["f_one_chunk_33_31"][1] == 1 and plan["f_one_chunk_33_32"][1] == 1
    assert plan["f_704_batch3_empty_chunks"] == (33, 32, 2)            # chunks 17 .. 31 receive no unit
    assert plan["f_704_batch1"] == (11, 11, 1)
    assert plan["g_mfma_32_32_49x129_65_units"] == (65, 64, 2)         # 33 chunks carry data
    for k, cfg in fr.KERNEL_CASES.items():                             # no entry of a weight gradient sums more
        assert cfg["batch"] * int(torch.tensor(cfg["dims"]).prod()) <= 8192, k


@pytest.mark.parametrize("name", [k for k in sorted(fr.KERNEL_CASES) if k.startswith("b_")]
                         + ["a_17x65_k7_periodic", "g_mfma_32_32_49x129_65_units"])
def test_one_gradient_alone_and_a_repeat_give_the_same_bits(name):
    cfg = fr.KERNEL_CASES[name]
    x, w, g = fr.case_inputs(cfg, 92)
    h = fr.grid_width_of(cfg)
    a, b = _run(cfg, x, w, g, h), _run(cfg, x, w, g, h)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    _, gx, none = _run(cfg, x, w, g, h, want_w=False)
    assert none is None and torch.equal(gx, a[1])
    _, none, gw = _run(cfg, x, w, g, h, want_x=False)
    assert none is None and torch.equal(gw, a[2])
