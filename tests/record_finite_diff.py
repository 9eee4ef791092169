"""Recorder of tests/golden/finite_diff_*.npz and tests/golden/sobolev_loss_*.npz -- run by hand where the reference
exists:

    python tests/record_finite_diff.py

Loads the verbatim ``neuralop/losses/differentiation.py`` and ``data_losses.py`` from where they lie and runs
``FiniteDiff``, ``LpLoss`` and ``H1Loss`` in float64 on fp32-representable inputs: every method's output and the
gradients for fixed cotangents (finite_diff_reference.run_all / run_losses).  Grids, spacings, periodic flags and loss
configurations: finite_diff_reference.CASES / LOSS_CASES / loss_configs."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import finite_diff_reference as fdr  # noqa: E402


def _save(name, rec):
    assert all(a.dtype == np.float64 for k, a in rec.items() if k.startswith("ref:"))
    path = os.path.join(fdr.GOLDEN, name + ".npz")
    np.savez(path, **rec)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KB")


def main():
    diff, losses = fdr.load_reference_losses()
    for seed, (name, (grid, h, periodic)) in enumerate(sorted(fdr.CASES.items())):
        dim = len(grid)
        g = torch.Generator().manual_seed(700 + seed)
        u32 = torch.randn(*fdr.LEAD, *grid, generator=g)
        v32 = torch.randn(*fdr.LEAD, dim, *grid, generator=g)
        u, v = u32.double().requires_grad_(True), v32.double().requires_grad_(True)
        fd = diff.FiniteDiff(dim, h=h if dim > 1 else h[0], **{"periodic_in_" + "xyz"[a]: periodic[a] for a in range(dim)})
        res = fdr.run_all(fd, u, v, 900 + seed, dim)
        rec = {"u": u32.numpy(), "v": v32.numpy(), "gseed": np.int64(900 + seed)}
        rec.update({"ref:" + k: t.numpy() for k, t in res.items()})
        _save(name, rec)
    classes = {"LpLoss": losses.LpLoss, "H1Loss": losses.H1Loss}
    for seed, (name, (shape, d, measure, np_flags)) in enumerate(sorted(fdr.LOSS_CASES.items())):
        g = torch.Generator().manual_seed(800 + seed)
        x32, y32 = torch.randn(*shape, generator=g), torch.randn(*shape, generator=g)
        x = x32.double().requires_grad_(True)
        res = fdr.run_losses(classes, x, y32.double(), name)
        rec = {"x": x32.numpy(), "y": y32.numpy()}
        rec.update({"ref:" + k: t.numpy() for k, t in res.items()})
        _save(name, rec)


if __name__ == "__main__":
    main()
