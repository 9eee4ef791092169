"""Recorder of tests/golden/fdconv_*.npz -- run by hand where the reference exists:

    python tests/record_fdconv.py

Loads the verbatim ``neuralop/layers/differential_conv.py`` by path and runs ``FiniteDifferenceConvolution`` in float64
on fp32-representable inputs, weights and cotangent (fdconv_reference.case_inputs): x, g, weight, grid_width, the
state-dict keys, float64 out / grad:x / grad:weight, and f32err:* = the rel-L2 error of the same class run in fp32
against its own float64 run (the bar of the smooth-field case is twice that).  The fp32 run's arrays themselves (f32:*)
are kept where the file stays below 200 KB.  Cases: fdconv_reference.CASES."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import fdconv_reference as fr  # noqa: E402


def run(cls, cfg, x, w, g, h, dtype):
    m = cls(**fr.module_kwargs(cfg)).to(dtype)
    with torch.no_grad():
        m.weight.copy_(w.to(dtype))
    xx = x.to(dtype).clone().requires_grad_(True)
    out = m(xx, h)
    out.backward(g.to(dtype))
    return m, {"out": out.detach().numpy(), "grad:x": xx.grad.numpy(), "grad:weight": m.weight.grad.numpy()}


def record(name, cfg, seed, cls):
    x, w, g = fr.case_inputs(cfg, seed)
    h = fr.grid_width_of(cfg)
    m, ref = run(cls, cfg, x, w, g, h, torch.float64)
    _, f32 = run(cls, cfg, x, w, g, h, torch.float32)
    assert all(v.dtype == np.float64 for v in ref.values())
    rec = {"x": x.numpy(), "g": g.numpy(), "weight": w.numpy(), "grid_width": np.float64(h), "seed": np.int64(seed),
           "state_keys": np.array(list(m.state_dict())), **ref}
    for k in ref:
        rec["f32err:" + k] = np.float64(fr.rel_l2(f32[k], ref[k]))
    if sum(v.nbytes for v in rec.values()) + sum(v.nbytes for v in f32.values()) < 200 * 1024:
        rec.update({"f32:" + k: v for k, v in f32.items()})
    path = os.path.join(fr.GOLDEN, "fdconv_" + name + ".npz")
    np.savez(path, **rec)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KB, fp32 errors " +
          " ".join(f"{k}={float(rec['f32err:' + k]):.1e}" for k in ref))


def main():
    cls = fr.load_reference_class()
    for i, (name, cfg) in enumerate(sorted(fr.CASES.items())):
        record(name, cfg, 5200 + i, cls)


if __name__ == "__main__":
    main()
