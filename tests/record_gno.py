"""Recorder of tests/golden/gno_*.npz -- run by hand where the reference exists:

    python tests/record_gno.py

Loads the verbatim ``neuralop/layers/gno_block.py`` (and through it neighbor_search.py, segment_csr.py,
integral_transform.py, channel_mlp.py, embeddings.py) and gno_weighting_functions.py from where they lie and runs
``GNOBlock`` in float64 on fp32-representable inputs and parameters with use_open3d=False and use_torch_scatter=False:
inputs, parameters, the neighbour dict, the output and the gradients for a fixed cotangent.  float64 matters: in fp32 the
reference's cdist switches to a matrix-product formula above 25 points and its boundary decisions become noise.  The
engine tests d2 <= r2 in fp32, the reference dist <= r: the recorder asserts that no pair lies within 1e-5 r of the
radius and otherwise moves on to the next seed, so that neighbour lists must match exactly.  Cases:
gno_reference.CASES."""
import os
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import gno_reference as gr  # noqa: E402


def record(name, cfg, base_seed, gno_block, wf):
    seed = base_seed
    while True:                                              # deterministic: the first seed without a pair in the band
        y32, x32, f32 = gr.case_inputs(cfg, seed)
        if not gr.band_queries(y32.numpy(), x32.numpy(), cfg["radius"]).any():
            break
        seed += 1000
    torch.manual_seed(seed)
    wfn = partial(wf.half_cos_cutoff, radius=cfg["radius"] ** 2, scale=1.0) if cfg["weighting"] == "half_cos" else None
    mlp_cls = sys.modules["neuralop.layers.channel_mlp"].LinearChannelMLP
    block = gno_block.GNOBlock(**gr.block_kwargs(cfg, wfn, mlp_cls)).double()
    with torch.no_grad():
        for p in block.parameters():
            p.copy_(p.float().double())
    y = y32.double()
    x = y if cfg["special"] == "x_is_y" else x32.double()
    f = None if f32 is None else f32.double().requires_grad_(True)
    nbrs = block.neighbor_search(data=y, queries=x, radius=cfg["radius"])
    out = block(y, x, f)
    g32 = torch.randn(*out.shape, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float32)
    out.backward(g32.double())
    rec = {"y": y32.numpy(), "x": x32.numpy(), "g": g32.numpy(), "seed": np.int64(seed),
           "ref:out": out.detach().numpy().astype(np.float64)}
    if f is not None:
        rec["f_y"] = f32.numpy()
        rec["ref:grad:f_y"] = f.grad.numpy()
    for k, v in nbrs.items():
        rec["nbr:" + k] = v.numpy()
    sd = block.state_dict()
    rec["state_keys"] = np.array(list(sd))
    rec["state_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
    for k, v in sd.items():
        rec["param:" + k] = v.float().numpy()
    for k, p in block.named_parameters():
        rec["ref:grad:" + k] = p.grad.numpy()
    assert all(a.dtype == np.float64 for k, a in rec.items() if k.startswith("ref:"))
    path = os.path.join(gr.GOLDEN, "gno_" + name + ".npz")
    np.savez(path, **rec)
    print(f"{name}: seed {seed}, {len(nbrs['neighbors_index'])} edges, {os.path.getsize(path) / 1024:.0f} KB")


def main():
    torch.set_default_dtype(torch.float64)                   # segment_csr's torch.zeros, the search's constants
    gno_block, wf = gr.load_reference_gno()
    for i, (name, cfg) in enumerate(sorted(gr.CASES.items())):
        record(name, cfg, 4100 + i, gno_block, wf)


if __name__ == "__main__":
    main()
