"""The recorded GNO cases (tests/golden/gno_*.npz, from the verbatim reference in float64) replayed with the kernel MLP on
its fused route -- engine.EdgeMlpFn, forced by gno.kernel_route("fused") without touching the block: on the
host-emulation build (CPU tier) and on the device (gpu).  Same bars as the edge route: neighbour dicts exactly, outputs
and f_y gradients to 1e-5, parameter gradients to 2e-5 (rel-L2).  The one case with a ReLU network is not eligible and
raises."""
import pytest
import torch

import gno_reference as gr
from conftest import load_golden
from emu_engine import engine_on_emulation

INELIGIBLE = "2d_linear_relu_custom_mlp"


def _replay(name, device):
    from neuraloperator_amd import engine
    from neuraloperator_amd.gno import kernel_route
    rec = load_golden("gno_" + name)
    before = engine.EdgeMlpFn.calls
    with kernel_route("fused"):
        if name == INELIGIBLE:
            with pytest.raises(ValueError, match="fused"):
                gr.run_engine_case(gr.CASES[name], rec, device)
            assert engine.EdgeMlpFn.calls == before
            return
        res = gr.run_engine_case(gr.CASES[name], rec, device)
    assert engine.EdgeMlpFn.calls == before + 1, "the fused route was not taken"
    errs = gr.check_case_against_record(res, rec)
    print(name, {k: f"{v:.1e}" for k, v in errs.items()})


def test_exactly_one_recorded_case_is_ineligible():
    assert [n for n, c in gr.CASES.items() if c["relu"]] == [INELIGIBLE] and len(gr.CASES) == 15


@pytest.mark.parametrize("name", sorted(gr.CASES))
def test_recorded_case_on_the_fused_route(name):
    with engine_on_emulation():
        _replay(name, torch.device("cpu"))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(gr.CASES))
def test_recorded_case_on_the_fused_route_on_the_device(name):
    _replay(name, torch.device("cuda:0"))
