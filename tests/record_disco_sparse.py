"""Recorder of tests/golden/dsparse_*.npz -- run by hand where the reference exists:

    python tests/record_disco_sparse.py

Loads the verbatim ``neuralop/layers/discrete_continuous_convolution.py`` by path (disco_reference.load_reference_module:
the stand-in torch_harmonics supplies the project's own filter basis), builds DiscreteContinuousConv2d /
DiscreteContinuousConvTranspose2d on the tensor grids of disco_sparse_reference.case_grids, keeps psi_idx / psi_vals as
the class built them (fp32, or float64 for float64 grids), and runs the module in float64 on fp32-representable x,
weight, bias and cotangent.  Each file holds the grids, q, x, g, weight, bias, the float64 out and the gradients
grad:x / grad:weight / grad:bias, psi_idx (as int32) and psi_vals, the attribute values and the state-dict keys; each
stays under 200 KB.  Cases: disco_sparse_reference.CASES."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import disco_sparse_reference as ds  # noqa: E402


def record(name, cfg, seed):
    grid_in, grid_out, q = ds.case_grids(cfg, seed)
    m = ds.reference_class(cfg["transposed"])(grid_in=grid_in, grid_out=grid_out, quadrature_weights=q, **cfg["kwargs"])
    psi_idx, psi_vals = m.psi_idx.detach().clone(), m.psi_vals.detach().clone()
    assert psi_vals.dtype == (torch.float64 if cfg["float64"] else torch.float32)
    assert int(psi_idx.max()) < 2 ** 31
    x, w, b, g = ds.case_inputs(cfg, m, seed)
    m = m.double()
    with torch.no_grad():
        m.weight.copy_(w.double())
        if b is not None:
            m.bias.copy_(b.double())
    xx = x.double().requires_grad_(True)
    out = m(xx)
    out.backward(g.double())
    rec = {"grid_in": grid_in.numpy(), "grid_out": grid_out.numpy(), "q": q.numpy(), "x": x.numpy(), "g": g.numpy(),
           "weight": w.numpy(), "out": out.detach().numpy(), "grad:x": xx.grad.numpy(),
           "grad:weight": m.weight.grad.numpy(), "psi_idx": psi_idx.numpy().astype(np.int32), "psi_vals": psi_vals.numpy(),
           "seed": np.int64(seed), "state_keys": np.array(list(m.state_dict())),
           "kernel_shape": np.array(m.kernel_shape, np.int64)}
    if b is not None:
        rec.update({"bias": b.numpy(), "grad:bias": m.bias.grad.numpy()})
    for a in ds.NUMERIC_ATTRS:
        rec["attr:" + a] = np.float64(getattr(m, a))
    if cfg["lonely"]:                                        # no neighbour: the bias alone
        assert np.array_equal(rec["out"][:, :, ds.LONELY], np.broadcast_to(b.double().numpy(), (cfg["batch"], b.numel())))
    path = ds.golden_path(name)
    np.savez(path, **rec)
    size = os.path.getsize(path)
    assert size < 200 * 1024, (name, size)
    print(f"{name}: {size / 1024:.0f} KB, {m.n_in} -> {m.n_out} points, K {m.kernel_size}, nnz {psi_vals.numel()}")


def main():
    for i, (name, cfg) in enumerate(sorted(ds.CASES.items())):
        record(name, cfg, 7300 + i)


if __name__ == "__main__":
    main()
