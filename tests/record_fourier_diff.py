"""Recorder of tests/golden/fourier_diff_*.npz -- run by hand where the reference exists:

    python tests/record_fourier_diff.py

Loads the verbatim ``neuralop/losses/differentiation.py`` from where it lies and runs its ``FourierDiff`` in float64
on fp32-representable inputs (float64 as the default dtype, so that its frequencies are float64 as well): every
method's output and ``u.grad`` / ``v.grad`` for fixed random cotangents (fourier_diff_reference.run_all).  Grids, unequal L per axis and low-pass ratios: fourier_diff_reference.CASES; two
leading dims (2, 3)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import fourier_diff_reference as fr  # noqa: E402


def main():
    ref = fr.load_reference_differentiation()
    for seed, (name, (grid, L, ratio)) in enumerate(sorted(fr.CASES.items())):
        dim = len(grid)
        g = torch.Generator().manual_seed(100 + seed)
        u32 = torch.randn(*fr.LEAD, *grid, generator=g)
        v32 = torch.randn(*fr.LEAD, dim, *grid, generator=g)
        u = u32.double().requires_grad_(True)
        v = v32.double().requires_grad_(True)
        fd = ref.FourierDiff(dim, L=L if dim > 1 else L[0], low_pass_filter_ratio=ratio)
        with fr.default_float64():                     # float64 frequencies too (fftfreq takes the default dtype)
            res = fr.run_all(fd, u, v, 500 + seed, dim)
        rec = {"u": u32.numpy(), "v": v32.numpy(), "gseed": np.int64(500 + seed)}
        rec.update({"ref:" + k: t.numpy() for k, t in res.items()})
        assert all(a.dtype == np.float64 for k, a in rec.items() if k.startswith("ref:"))
        path = os.path.join(fr.GOLDEN, name + ".npz")
        np.savez(path, **rec)
        print(f"{name}: {os.path.getsize(path) / 1024:.0f} KB")


if __name__ == "__main__":
    main()
