"""Recorder of tests/golden/sproj_*.npz -- run by hand where the reference exists:

    python tests/record_spectral_projection.py

Loads the verbatim ``neuralop/layers/spectral_projection.py`` from where it lies and runs its
``spectral_projection_divergence_free`` in float64 on fp32-representable inputs (float64 as the default dtype, so that
its wavenumbers are float64 as well): the output, ``u.grad`` for a fixed random cotangent, and -- as ``err:fp32`` -- the
rel-L2 of the same function run in fp32 against that output (what fp32 costs the reference itself).  Grids, domain
sizes and mode counts: spectral_projection_reference.CASES; batch 2."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import spectral_projection_reference as pr  # noqa: E402


def main():
    ref = pr.load_reference_projection()
    for seed, (name, (grid, domain, modes)) in enumerate(sorted(pr.CASES.items())):
        g = torch.Generator().manual_seed(300 + seed)
        u32 = torch.randn(pr.BATCH, 2, *grid, generator=g)
        u = u32.double().requires_grad_(True)
        with pr.default_float64():                     # float64 wavenumbers too (fftfreq takes the default dtype)
            res = pr.run_case(ref, u, domain, modes, 700 + seed)
        own = ref(u32, domain, modes)
        rec = {"u": u32.numpy(), "gseed": np.int64(700 + seed), "err:fp32": np.float64(pr.rel_l2(own, res["out"]))}
        rec.update({"ref:" + k: t.numpy() for k, t in res.items()})
        assert all(a.dtype == np.float64 for k, a in rec.items() if k.startswith("ref:"))
        path = os.path.join(pr.GOLDEN, name + ".npz")
        np.savez(path, **rec)
        print(f"{name}: {os.path.getsize(path) / 1024:.1f} KB, fp32 reference {float(rec['err:fp32']):.1e}")


if __name__ == "__main__":
    main()
