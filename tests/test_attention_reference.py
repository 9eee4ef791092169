"""CPU tier: AttentionKernelIntegral / RotaryEmbedding2D against fixtures recorded from the verbatim reference classes
(tests/record_attention.py, tests/golden/attn_*.npz), the engine in host emulation: bit-equal initial parameters, state
dict keys and attributes, the error texts, out and every gradient to the bar of attention_reference.tolerance (1e-5
rel-L2 of the float64 record), the route actually taken, the torch path for float64, associative=False (with the
kernel matrix), a foreign embedding module and CPU tensors without the emulation, and the reference's two shape
failures."""
import numpy as np
import pytest
import torch

import attention_reference as ar
from emu_engine import engine_on_emulation
from neuraloperator_amd import AttentionKernelIntegral, RotaryEmbedding2D, attention

NAMES = sorted(ar.CASES)


@pytest.fixture
def emu():                                                   # per test: the fallback tests run without it
    with engine_on_emulation() as lib:
        yield lib


@pytest.fixture(scope="module")
def records():
    return {name: ar.load_record(name) for name in NAMES}


def _build(name):
    return ar.build_layer(AttentionKernelIntegral, RotaryEmbedding2D, ar.CASES[name], ar.SEEDS[name])


def _inputs(rec, dtype=torch.float32):
    t = {k: torch.from_numpy(rec[k]).to(dtype) for k in ("u_src", "pos_src", "u_qry", "pos_qry", "weights", "g")
         if k in rec}
    for k in ("u_src", "u_qry"):
        if k in t:
            t[k].requires_grad_(True)
    return t


def _check(name, rec, out, grads):
    errs = {"out": ar.rel_l2(out.detach().numpy(), rec["out"])}
    for k, g in grads.items():
        assert g is not None, k
        errs["grad:" + k] = ar.rel_l2(g.numpy(), rec["grad:" + k])
    assert set(errs) == {k for k in rec if k == "out" or k.startswith("grad:")}
    print(name, " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= ar.tolerance(rec, k), (k, e)


@pytest.mark.parametrize("name", NAMES)
def test_initial_parameters_keys_and_attributes(records, name):
    cfg, rec = ar.CASES[name], records[name]
    m, emb = _build(name)
    state = m.state_dict()
    assert list(state) == [str(k) for k in rec["state_keys"]]
    for k, v in state.items():
        assert v.dtype == torch.float32 and np.array_equal(v.numpy(), rec["state:" + k]), k
    t = ar.case_inputs(cfg, int(rec["seed"]))                            # the record is what the case table says
    assert all(np.array_equal(v.numpy(), rec[k]) for k, v in t.items())
    assert (m.n_heads, m.head_n_channels, m.in_channels, m.out_channels, m.project_query) == \
        (cfg["heads"], cfg["d"], cfg["in_channels"], cfg["out_channels"], cfg["project_query"])
    assert m.init_gain == m.diagonal_weight == 1 / np.sqrt(cfg["d"])
    assert isinstance(m.to_q, torch.nn.Linear if cfg["project_query"] else torch.nn.Identity)
    assert isinstance(m.to_out, torch.nn.Identity if cfg["heads"] * cfg["d"] == cfg["out_channels"] else torch.nn.Linear)
    assert isinstance(m.k_norm, torch.nn.InstanceNorm1d) and isinstance(m.v_norm, torch.nn.InstanceNorm1d)
    if emb is not None:
        assert emb.out_channels == 2 and "inv_freq" not in emb.state_dict()
        assert emb.inv_freq.numel() == cfg["d"] // (2 * cfg["pos_dim"]) and (emb.min_freq, emb.scale) == (1 / 64, 1.0)


def test_the_case_table_covers_the_forms():
    c = ar.CASES.values()
    assert {4, 12, 32, 64} <= {x["d"] for x in c} and {1, 3} <= {x["heads"] for x in c}
    assert any(x["d"] == x["in_channels"] for x in c) and any(x["d"] != x["in_channels"] for x in c)
    assert any(x["pos_dim"] == 1 and x["batch"] == 1 for x in c) and any(not x["rotary"] for x in c)
    assert any(x["cross"] and x["rotary"] for x in c) and any(x["cross"] and not x["rotary"] for x in c)
    assert any(x["weights"] for x in c) and any(not x["project_query"] for x in c)
    assert max(x["n"] for x in c) <= 96


@pytest.mark.parametrize("name", NAMES)
def test_engine_route_against_the_record(emu, records, name):
    rec = records[name]
    m, emb = _build(name)
    t = _inputs(rec)
    args = dict(positional_embedding_module=emb, u_qry=t.get("u_qry"), pos_qry=t.get("pos_qry"), weights=t.get("weights"))
    assert m.on_engine(t["u_src"], t["pos_src"], **args)
    with attention.route("engine"):
        out = ar.call_layer(m, emb, t)
    out.backward(t["g"])
    _check(name, rec, out, ar.grads_of(m, t))


@pytest.mark.parametrize("name", ["self_rot2_unit_positions_d12", "cross_weights_no_query_projection_d4",
                                  "self_rot1_batch1_d12"])
def test_torch_path_on_cpu_tensors_and_in_float64(records, name):
    """without the emulation CPU tensors take the torch formula; so does float64 anywhere"""
    rec = records[name]
    m, emb = _build(name)
    t = _inputs(rec)
    assert not m.on_engine(t["u_src"], t["pos_src"], positional_embedding_module=emb, u_qry=t.get("u_qry"),
                           pos_qry=t.get("pos_qry"), weights=t.get("weights"))
    out = ar.call_layer(m, emb, t)
    out.backward(t["g"])
    _check(name, rec, out, ar.grads_of(m, t))
    with attention.route("engine"), pytest.raises(ValueError, match="not eligible"):
        ar.call_layer(m, emb, t)
    m64, emb64 = _build(name)
    m64, emb64, t64 = m64.double(), None if emb64 is None else emb64.double(), _inputs(rec, torch.float64)
    with engine_on_emulation():
        assert not m64.on_engine(t64["u_src"], t64["pos_src"], positional_embedding_module=emb64,
                                 u_qry=t64.get("u_qry"), pos_qry=t64.get("pos_qry"), weights=t64.get("weights"))
        out = ar.call_layer(m64, emb64, t64)
    out.backward(t64["g"])
    assert out.dtype == torch.float64
    for k, g in [("out", out.detach())] + [("grad:" + k, g) for k, g in ar.grads_of(m64, t64).items()]:
        assert ar.rel_l2(g.numpy(), rec[k]) <= (1e-7 if ar.CASES[name]["compact"] else 1e-12), k


@pytest.mark.parametrize("name", [n for n in NAMES if ar.CASES[n]["kernel"]])
def test_non_associative_form_and_its_kernel_matrix(emu, records, name):
    rec = records[name]
    m, emb = _build(name)
    t = _inputs(rec)
    assert not m.on_engine(t["u_src"], t["pos_src"], positional_embedding_module=emb, associative=False)
    out, kxy = ar.call_layer(m, emb, t, associative=False, return_kernel=True)
    assert ar.rel_l2(kxy.detach().numpy(), rec["kernel"]) <= ar.tolerance(rec, "kernel")
    out.backward(t["g"])
    _check(name, rec, out, ar.grads_of(m, t))


class _ForeignEmbedding(torch.nn.Module):
    """not the reference's class: the same angles from other attributes"""

    def __init__(self, dim):
        super().__init__()
        self.inner = RotaryEmbedding2D(dim)
        self.apply_1d_rotary_pos_emb = RotaryEmbedding2D.apply_1d_rotary_pos_emb
        self.apply_2d_rotary_pos_emb = RotaryEmbedding2D.apply_2d_rotary_pos_emb

    def forward(self, coordinates):
        return self.inner(coordinates)


def test_a_foreign_embedding_module_takes_the_torch_path(emu, records):
    name = "self_rot2_unit_positions_d12"
    rec, cfg = records[name], ar.CASES[name]
    m, _ = _build(name)
    emb = _ForeignEmbedding(cfg["d"] // 2)
    t = _inputs(rec)
    assert not m.on_engine(t["u_src"], t["pos_src"], positional_embedding_module=emb)
    out = ar.call_layer(m, emb, t)
    out.backward(t["g"])
    _check(name, rec, out, ar.grads_of(m, t))
    # the reference's class with an inv_freq of another length is not the engine's either
    assert not m.on_engine(t["u_src"], t["pos_src"], positional_embedding_module=RotaryEmbedding2D(cfg["d"]))
    # positions or weights that need a gradient stay in torch
    assert not m.on_engine(t["u_src"], t["pos_src"].clone().requires_grad_(True),
                           positional_embedding_module=RotaryEmbedding2D(cfg["d"] // 2))
    assert m.on_engine(t["u_src"], t["pos_src"], positional_embedding_module=RotaryEmbedding2D(cfg["d"] // 2))
    with attention.route("torch"):
        assert not m.on_engine(t["u_src"], t["pos_src"], positional_embedding_module=RotaryEmbedding2D(cfg["d"] // 2))
    with pytest.raises(ValueError, match="route must be one of"):
        with attention.route("fast"):
            pass


def test_error_texts():
    m = AttentionKernelIntegral(8, 8, 2, 4)
    x, pos = torch.randn(2, 5, 8), torch.rand(2, 5, 2)
    with pytest.raises(ValueError) as e:
        m(x, pos, pos_qry=pos)
    assert str(e.value) == "Query coordinates are provided but query function is not provided"
    with pytest.raises(ValueError) as e:
        m(x, pos, u_qry=x)
    assert str(e.value) == "Query coordinates are required if query function is provided"
    with pytest.raises(ValueError) as e:
        m(x, pos, return_kernel=True)
    assert str(e.value) == "Cannot get kernel matrix when associative is set to True"
    with pytest.raises(ValueError) as e:
        m(x, torch.rand(2, 5, 3), positional_embedding_module=RotaryEmbedding2D(2))
    assert str(e.value) == "Currently doesnt support relative embedding >= 3 dimensions"


def test_the_two_shape_failures_of_the_reference(emu):
    m = AttentionKernelIntegral(8, 8, 2, 4)
    x, pos = torch.randn(2, 6, 8), torch.rand(2, 6, 2)
    xq, pq = torch.randn(2, 9, 8), torch.rand(2, 9, 2)
    assert not m.on_engine(x, pos, u_qry=xq, pos_qry=pq)
    with pytest.raises(RuntimeError, match="shape|size|view"):           # n_qry != n_src dies in the final view
        m(x, pos, u_qry=xq, pos_qry=pq)
    emb = RotaryEmbedding2D(4)
    assert not m.on_engine(x, pos[..., :1], positional_embedding_module=emb)
    with pytest.raises(RuntimeError, match="size of tensor|must match"):  # 1-d rotary with batch > 1 dies in the repeat
        m(x, pos[..., :1], positional_embedding_module=emb)
    assert m.on_engine(x[:1], pos[:1, :, :1], positional_embedding_module=emb)


def test_the_fp32_formula_alone_holds_the_row_bounds_on_the_whole_kernel_table():
    """no engine: the plain formula with every tensor in fp32 (ar.manual_core; its layer-norm backward in float64, as the
    kernels' own) against the float64 helper on every ar.ATTN_KERNEL_CASES entry -- rel-L2 <= 1e-5 per tensor and
    ||err_row|| <= 1e-5 ||A_row|| per row (level 1 of DESIGN 3.26), so no case is too ill-conditioned for the bar; and the
    same chain in float64 equals the autograd helper, so the two statements of the formula agree"""
    worst = {}
    for name, cfg in ar.ATTN_KERNEL_CASES.items():
        args, ref = ar.kernel_reference(name)
        common = args[:8] + (cfg["heads"], cfg["rotary"], args[8])
        again = ar.manual_core(*common, torch.float64)
        assert set(again) == set(ar.TENSORS)
        for key, t in again.items():
            assert ar.rel_l2(t.numpy(), ref[key][0].numpy()) <= 1e-12, (name, key)
            assert bool((ref[key][1] >= ref[key][0].abs() * (1 - 1e-12)).all()), (name, key)     # A >= |value|
        stats = ar.check_levels(name, cfg, ar.manual_core(*common, torch.float32), ref, element=False)
        for key, (rel, row, _) in stats.items():
            worst[key] = max(worst.get(key, (0.0, 0.0)), (row, rel))
    print("worst (row ratio, rel-L2) of the fp32 formula:", {k: (round(a, 3), float(f"{b:.1e}")) for k, (a, b) in worst.items()})
