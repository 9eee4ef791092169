"""CPU tier: neuraloperator_amd.FiniteDifferenceConvolution on the host-emulation build against fixtures recorded from
the verbatim reference in float64 (tests/record_fdconv.py, tests/golden/fdconv_*.npz): out, grad:x and grad:weight to
1e-5 rel-L2; on the smooth field, where the stencil cancels, to twice the verbatim fp32 class's own error against its
float64 run.  State-dict layout, constructor errors, the torch fallback; where the reference exists, checkpoints both
ways, and the float64 helper of tests/fdconv_reference.py against the live class to 1e-12.

Measured on the emulation build (rel-L2 of out / grad:x / grad:weight), smooth field: 1.84e-07 / 1.64e-07 / 1.94e-07
against bars of 5.28e-07 / 3.61e-07 / 8.60e-07, i.e. 0.70 / 0.91 / 0.45 of the verbatim fp32 class's own error."""
import numpy as np
import pytest
import torch

import fdconv_reference as fr
from conftest import load_golden
from emu_engine import engine_on_emulation

needs_reference = pytest.mark.skipif(not fr.reference_available(), reason="the verbatim reference is not on this machine")
CPU = torch.device("cpu")


def test_the_class_imports_from_the_package():
    from neuraloperator_amd import FiniteDifferenceConvolution  # noqa: F401


def _record_inputs(rec):
    return torch.from_numpy(rec["x"]), torch.from_numpy(rec["weight"]), torch.from_numpy(rec["g"]), float(rec["grid_width"])


@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_layer_matches_the_recorded_reference(name):
    cfg, rec = fr.CASES[name], load_golden("fdconv_" + name)
    x, w, g, h = _record_inputs(rec)
    with engine_on_emulation():
        out, gx, gw, m = fr.run_module(cfg, x, w, g, h, CPU)
    bars = fr.record_bars(cfg, rec)
    got, want = (out, gx, gw), (rec["out"], rec["grad:x"], rec["grad:weight"])
    raw = tuple(fr.rel_l2(a, b) for a, b in zip(got, want))
    print(name, "errors", " ".join(f"{e:.2e}" for e in raw), "bars", " ".join(f"{b:.2e}" for b in bars))
    if cfg["smooth"]:
        print(name, "ratio to the verbatim fp32 class's own error",
              " ".join(f"{2 * e / b:.2f}" for e, b in zip(raw, bars)))
    fr.check_against(cfg, got, want, bars, fr.magnitudes(x, w, g, h, cfg["groups"], cfg["padding"]))
    assert sorted(m.state_dict()) == sorted(str(k) for k in rec["state_keys"])


def test_state_dict_layout_and_constructor_errors():
    from neuraloperator_amd import FiniteDifferenceConvolution
    m = FiniteDifferenceConvolution(6, 4, 2, kernel_size=5, groups=2, padding="reflect")
    assert (m.kernel_size, m.in_channels, m.groups, m.n_dim, m.padding_mode, m.pad_size) == (5, 6, 2, 2, "reflect", 2)
    assert isinstance(m.conv, torch.nn.Conv2d) and m.weight is m.conv.weight and m.conv.bias is None
    assert tuple(m.weight.shape) == (4, 3, 5, 5)
    assert list(m.state_dict()) == ["weight", "conv.weight"]
    assert [k for k, _ in m.named_parameters()] == ["weight"]
    assert FiniteDifferenceConvolution(2, 2, 1).padding_mode == "circular"
    assert FiniteDifferenceConvolution(2, 2, 3, padding="zeros").padding_mode == "zeros"
    assert FiniteDifferenceConvolution(2, 2, 3, padding="replicate").padding_mode == "replicate"
    with pytest.raises(AssertionError, match="Kernel size should be odd"):
        FiniteDifferenceConvolution(2, 2, 2, kernel_size=4)
    with pytest.raises(NotImplementedError, match="not currently supported"):
        FiniteDifferenceConvolution(2, 2, 2, padding="wrap")
    # the same initialisation as torch's own convolution under the same seed
    torch.manual_seed(3)
    a = FiniteDifferenceConvolution(4, 6, 2, groups=2).weight.detach().clone()
    torch.manual_seed(3)
    b = torch.nn.Conv2d(4, 6, 3, groups=2, bias=False).weight.detach()
    assert torch.equal(a, b)


@pytest.mark.parametrize("case", ["float64", "tensor_grid_width", "k9", "4d"])
def test_torch_fallback_equals_the_formula(case):
    from neuraloperator_amd import FiniteDifferenceConvolution
    g = torch.Generator().manual_seed(9)
    if case == "4d":
        with pytest.raises(AttributeError):
            FiniteDifferenceConvolution(2, 2, 4)              # torch has no Conv4d, as in the reference
        return
    k = 9 if case == "k9" else 3
    dtype = torch.float64 if case == "float64" else torch.float32
    m = FiniteDifferenceConvolution(4, 6, 2, kernel_size=k, groups=2, padding="replicate").to(dtype)
    x = torch.randn(2, 4, 11, 12, generator=g, dtype=dtype).requires_grad_(True)
    h = torch.tensor(0.05, dtype=dtype, requires_grad=True) if case == "tensor_grid_width" else 0.05
    assert not m.on_engine(x, h)
    out = m(x, h)                                            # no engine is loaded here: the torch formula ran
    gout = torch.randn(out.shape, generator=g, dtype=dtype)
    out.backward(gout)
    want = fr.fdconv_with_grads(x, m.weight, gout, 0.05, 2, "replicate")
    tol = 1e-12 if dtype == torch.float64 else 1e-5
    assert fr.rel_l2(out.detach().numpy(), want[0].numpy()) <= tol
    assert fr.rel_l2(x.grad.numpy(), want[1].numpy()) <= tol
    assert fr.rel_l2(m.weight.grad.numpy(), want[2].numpy()) <= tol
    if case == "tensor_grid_width":
        want_gh = -(want[0] * gout.double()).sum() / 0.05
        assert abs(float(h.grad) - float(want_gh)) <= 1e-4 * abs(float(want_gh))


def test_non_contiguous_input_and_no_weight_gradient():
    from neuraloperator_amd import FiniteDifferenceConvolution
    cfg = fr.CASES["2d_k3_replicate_g2"]
    x, w, g = fr.case_inputs(cfg, 31)
    h = fr.grid_width_of(cfg)
    m = FiniteDifferenceConvolution(**fr.module_kwargs(cfg))
    with torch.no_grad():
        m.weight.copy_(w)
    m.weight.requires_grad_(False)
    xt = x.transpose(2, 3).contiguous().transpose(2, 3).requires_grad_(True)
    assert not xt.is_contiguous()
    with engine_on_emulation():
        out = m(xt, h)
        out.backward(g)
    want = fr.fdconv_with_grads(x, w, g, h, cfg["groups"], cfg["padding"])
    assert fr.rel_l2(out.detach().numpy(), want[0].numpy()) <= 1e-5
    assert fr.rel_l2(xt.grad.numpy(), want[1].numpy()) <= 1e-5
    assert m.weight.grad is None


@needs_reference
def test_checkpoints_load_both_ways_with_the_verbatim_class():
    from neuraloperator_amd import FiniteDifferenceConvolution
    ref_cls = fr.load_reference_class()
    kw = dict(in_channels=6, out_channels=4, n_dim=3, kernel_size=3, groups=2, padding="zeros")
    torch.manual_seed(1)
    mine = FiniteDifferenceConvolution(**kw)
    torch.manual_seed(2)
    ref = ref_cls(**kw)
    assert list(mine.state_dict()) == list(ref.state_dict())
    assert [k for k, _ in mine.named_parameters()] == [k for k, _ in ref.named_parameters()]
    assert not torch.equal(mine.weight, ref.weight)
    ref.load_state_dict(mine.state_dict(), strict=True)
    assert torch.equal(ref.weight, mine.weight) and torch.equal(ref.conv.weight, mine.weight)
    torch.manual_seed(4)
    other = ref_cls(**kw)
    mine.load_state_dict(other.state_dict(), strict=True)
    assert torch.equal(mine.weight, other.weight) and mine.weight is mine.conv.weight
    for attr in ("kernel_size", "in_channels", "groups", "n_dim", "padding_mode", "pad_size"):
        assert getattr(mine, attr) == getattr(ref, attr), attr


@needs_reference
@pytest.mark.parametrize("name", sorted(fr.CASES))
def test_live_reference_helper_and_fixtures_agree(name):
    cfg, rec = fr.CASES[name], load_golden("fdconv_" + name)
    x, w, g, h = _record_inputs(rec)
    m = fr.load_reference_class()(**fr.module_kwargs(cfg)).double()
    with torch.no_grad():
        m.weight.copy_(w.double())
    xx = x.double().requires_grad_(True)
    out = m(xx, h)
    out.backward(g.double())
    live = (out.detach().numpy(), xx.grad.numpy(), m.weight.grad.numpy())
    helper = [t.numpy() for t in fr.fdconv_with_grads(x, w, g, h, cfg["groups"], cfg["padding"])]
    scales = fr.magnitudes(x, w, g, h, cfg["groups"], cfg["padding"])
    for a, b, key, s in zip(live, helper, ("out", "grad:x", "grad:weight"), scales):
        assert fr.rel_l2(a, rec[key], s) <= 1e-12, key      # the fixtures are what the reference computes
        assert fr.rel_l2(b, a, s) <= 1e-12, key
