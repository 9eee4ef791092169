"""Recorder of tests/golden/disco_*.npz -- run by hand where the reference exists:

    python tests/record_disco.py

Loads the verbatim ``neuralop/layers/discrete_continuous_convolution.py`` by path (disco_reference.load_reference_module:
the stand-in torch_harmonics supplies the project's own filter basis) and runs the two equidistant classes in float64 on
fp32-representable inputs, weights, bias and cotangent.  Each file holds x, g, weight, bias, the float64 out and the
gradients grad:x / grad:weight / grad:bias, the attribute values, the output shape, the filter buffer as the class built
it (fp32) and the state-dict keys; each stays under 200 KB.  Cases: disco_reference.CASES."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import disco_reference as dr  # noqa: E402


def record(name, cfg, seed):
    m = dr.reference_class(cfg["transposed"])(**cfg["kwargs"])
    buf = m.local_filter_matrix.detach().clone()
    assert buf.dtype == torch.float32
    x, w, b = dr.case_inputs(cfg, m, seed)
    m = m.double()
    with torch.no_grad():
        m.weight.copy_(w.double())
        if b is not None:
            m.bias.copy_(b.double())
    xx = x.double().requires_grad_(True)
    out = m(xx)
    g = dr.cotangent(out.shape, seed)
    out.backward(g.double())
    rec = {"x": x.numpy(), "g": g.numpy(), "weight": w.numpy(), "out": out.detach().numpy(), "grad:x": xx.grad.numpy(),
           "grad:weight": m.weight.grad.numpy(), "local_filter_matrix": buf.numpy(),
           "out_shape": np.array(out.shape, np.int64), "seed": np.int64(seed),
           "state_keys": np.array(list(m.state_dict())), "padding_mode": np.array(m.padding_mode),
           "kernel_shape": np.array(m.kernel_shape, np.int64), "domain_length": np.array(m.domain_length, np.float64)}
    if b is not None:
        rec.update({"bias": b.numpy(), "grad:bias": m.bias.grad.numpy()})
    for a in dr.NUMERIC_ATTRS:
        rec["attr:" + a] = np.float64(getattr(m, a))
    for k, v in cfg["expect"].items():
        assert getattr(m, k) == v, (name, k, getattr(m, k), v)
    path = os.path.join(dr.GOLDEN, "disco_" + name + ".npz")
    np.savez(path, **rec)
    size = os.path.getsize(path)
    assert size < 200 * 1024, (name, size)
    print(f"{name}: {size / 1024:.0f} KB, support {m.psi_local_h} x {m.psi_local_w}, K {m.kernel_size}, "
          f"out {tuple(out.shape)}")


def main():
    for i, (name, cfg) in enumerate(sorted(dr.CASES.items())):
        record(name, cfg, 6100 + i)


if __name__ == "__main__":
    main()
