"""CPU tier: neuraloperator_amd.NeighborSearch / IntegralTransform / GNOBlock on the host-emulation build against
fixtures recorded from the verbatim reference in float64 (tests/record_gno.py, tests/golden/gno_*.npz): neighbour dicts
exactly, outputs and f_y gradients to 1e-5, parameter gradients to 2e-5 (rel-L2), state-dict keys and shapes.  Where the
reference exists, the float64 helper of tests/gno_reference.py and the live reference agree to 1e-12."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gno_reference as gr
from conftest import load_golden
from emu_engine import engine_on_emulation

needs_reference = pytest.mark.skipif(not gr.reference_available(), reason="the verbatim reference is not on this machine")


def test_the_classes_import_from_the_package():
    from neuraloperator_amd import GNOBlock, IntegralTransform, NeighborSearch, segment_csr  # noqa: F401


@pytest.mark.parametrize("name", sorted(gr.CASES))
def test_gno_block_matches_the_recorded_reference(name):
    rec = load_golden("gno_" + name)
    with engine_on_emulation():
        res = gr.run_engine_case(gr.CASES[name], rec, torch.device("cpu"))
    errs = gr.check_case_against_record(res, rec)
    print(name, {k: f"{v:.1e}" for k, v in errs.items()})
    if gr.CASES[name]["special"] == "empty":
        rs = rec["nbr:neighbors_row_splits"]
        assert rs[3] == rs[2] and not res["out"][:, 2].any()


def test_segment_csr_and_error_paths():
    from neuraloperator_amd import GNOBlock, IntegralTransform, segment_csr
    rng = np.random.default_rng(3)
    splits, _ = gr.random_csr(rng, 5, 4, np.array([2, 0, 70, 1, 3]))
    src = torch.from_numpy(rng.standard_normal((2, int(splits[-1]), 6)).astype(np.float32))
    with engine_on_emulation():
        for red in ("sum", "mean"):
            for s in (src, src[0]):
                s = s.clone().requires_grad_(True)
                ind = torch.from_numpy(splits)
                out = segment_csr(s, ind if s.ndim == 2 else ind.unsqueeze(0).repeat(2, 1), red, use_scatter=False)
                ref = gr.csr_reduce(s.detach().numpy(), splits, mean=red == "mean")
                assert gr.rel_l2(out.detach().numpy(), ref) < 1e-6
                g = torch.from_numpy(rng.standard_normal(out.shape).astype(np.float32))
                out.backward(g)
                s64 = s.detach().double().requires_grad_(True)
                lens = np.diff(splits)
                rep = torch.repeat_interleave(torch.arange(5), torch.from_numpy(lens))
                o64 = torch.zeros(*s64.shape[:-2], 5, 6, dtype=torch.float64).index_add(-2, rep, s64)
                if red == "mean":
                    o64 = o64 / torch.from_numpy(np.maximum(lens, 1)).double().unsqueeze(-1)
                o64.backward(g.double())
                assert gr.rel_l2(s.grad.numpy(), s64.grad.numpy()) < 1e-6
        with pytest.raises(ValueError, match="reduce must be one of 'mean', 'sum'"):
            segment_csr(src, torch.from_numpy(splits), "max")
        with pytest.raises(ValueError, match="Got transform_type=cubic"):
            IntegralTransform(channel_mlp_layers=[4, 3], transform_type="cubic")
        with pytest.raises(AssertionError):
            IntegralTransform()
        with pytest.raises(AssertionError):
            GNOBlock(2, 2, coord_dim=2, radius=0.1)          # the open3d flag asks for 3-d, as in the reference
        it = IntegralTransform(channel_mlp_layers=[4, 8, 3], weighting_fn=lambda w: w)
        y = torch.rand(6, 2)
        nb = {"neighbors_index": torch.tensor([0, 1, 2], dtype=torch.int64),
              "neighbors_row_splits": torch.tensor([0, 1, 1, 2, 2, 3, 3], dtype=torch.int64)}
        with pytest.raises(KeyError, match="your neighborhoods must contain weights"):
            it(y, nb)
        with pytest.raises(NotImplementedError):
            it(y, nb, weights=torch.ones(3, requires_grad=True))
        with pytest.raises(ValueError):
            it(y, {**nb, "neighbors_row_splits": nb["neighbors_row_splits"][:-1]})
        # a user-built neighbour dict with per-edge weights through the generic and the lift route
        it2 = IntegralTransform(channel_mlp_layers=[4, 8, 3], channel_mlp_non_linearity=F.relu)
        assert it.lift_route() and not it2.lift_route()
        it2.load_state_dict(it.state_dict())
        w = torch.tensor([0.5, 2.0, 3.0])
        with torch.no_grad():
            a, b = it(y, nb, weights=w), it2(y, nb, weights=w)
        Ws = [p.double() for k, p in it.state_dict().items() if k.endswith("weight")]
        bs = [p.double() for k, p in it.state_dict().items() if k.endswith("bias")]
        nb64 = {**nb, "weights": w.double()}
        assert gr.rel_l2(a.numpy(), gr.integral_transform(y.double(), y.double(), nb64, Ws, bs).numpy()) < 1e-5
        assert gr.rel_l2(b.numpy(), gr.integral_transform(y.double(), y.double(), nb64, Ws, bs, act=F.relu).numpy()) < 1e-5


def test_reference_checkpoint_keys_of_the_default_block():
    from neuraloperator_amd import GNOBlock
    sd = GNOBlock(in_channels=2, out_channels=12, coord_dim=3, radius=0.035).state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == {
        f"integral_transform.channel_mlp.fcs.{i}.{p}": s
        for i, (o, n) in enumerate([(128, 384), (256, 128), (128, 256), (12, 128)])
        for p, s in (("weight", (o, n)), ("bias", (o,)))}   # the layer sizes the reference's docstring prints


@needs_reference
@pytest.mark.parametrize("name", sorted(gr.CASES))
def test_live_reference_helper_and_fixtures_agree(name):
    from functools import partial
    cfg, rec = gr.CASES[name], load_golden("gno_" + name)
    gno_block, wf = gr.load_reference_gno()
    import sys
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        wfn = partial(wf.half_cos_cutoff, radius=cfg["radius"] ** 2, scale=1.0) if cfg["weighting"] else None
        block = gno_block.GNOBlock(**gr.block_kwargs(cfg, wfn, sys.modules["neuralop.layers.channel_mlp"].LinearChannelMLP))
        block.load_state_dict({k[6:]: torch.from_numpy(v).double() for k, v in rec.items() if k.startswith("param:")})
        y = torch.from_numpy(rec["y"]).double()
        x = y if cfg["special"] == "x_is_y" else torch.from_numpy(rec["x"]).double()
        f = torch.from_numpy(rec["f_y"]).double() if "f_y" in rec else None
        nbrs = block.neighbor_search(data=y, queries=x, radius=cfg["radius"])
        out = block(y, x, f).detach()
        ye, xe = (block.pos_embedding(y), block.pos_embedding(x)) if block.pos_embedding is not None else (y, x)
    finally:
        torch.set_default_dtype(old)
    assert gr.rel_l2(out.numpy(), rec["ref:out"]) <= 1e-12  # the fixtures are what the reference computes
    mine = gr.radius_search(rec["y"], x.numpy(), cfg["radius"], cfg["weighting"] is not None)
    for k, v in nbrs.items():
        np.testing.assert_array_equal(v.numpy(), rec["nbr:" + k])
        if k == "weights":
            assert gr.rel_l2(mine[k], v.numpy()) <= 1e-12
        else:
            np.testing.assert_array_equal(mine[k], v.numpy())
    # the dense float64 helper on the embedded points
    sd = block.state_dict()
    Ws, bs = [v for k, v in sd.items() if k.endswith("weight")], [v for k, v in sd.items() if k.endswith("bias")]
    wfn64 = partial(gr.half_cos, radius=cfg["radius"] ** 2) if cfg["weighting"] else None
    h = gr.integral_transform(ye, xe, nbrs, Ws, bs, f_y=f, transform_type=cfg["transform_type"],
                              reduction=cfg["reduction"], weighting_fn=wfn64, act=F.relu if cfg["relu"] else F.gelu)
    assert gr.rel_l2(h.numpy(), rec["ref:out"]) <= 1e-12
