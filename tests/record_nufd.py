"""Record tests/golden/nufd_<case>.npz from the verbatim reference (run by hand where the reference exists):

    python tests/record_nufd.py

Per case of nufd_reference.CASES: the inputs (points, values, cotangent g -- fp32-representable, g zeroed at the excluded
points so that the recorded gradient comes from the compared stencils alone), what the reference's
``get_non_uniform_fd_weights`` / ``non_uniform_fd`` compute from them in float64 under ``ref:`` (indices, weights --
rounded to fp32 where the file would pass 200 KB --, derivatives, grad:values), under ``err:<tensor>`` the error of the
verbatim function run in fp32 against its float64 run (included points), and under ``err:model`` the error of the
apply's model: float64 weights rounded to fp32, times fp32 values, summed in float64.  Asserts that the helper's closed
form matches the float64 reference on the included points and that at most 1 % of the points are excluded."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fourier_diff_reference as fr  # noqa: E402
import nufd_reference as nr  # noqa: E402


def run_reference(mod, cfg, points, values, g, dtype):
    p = torch.from_numpy(points).to(dtype)
    v = torch.from_numpy(values).to(dtype).requires_grad_()
    kw = dict(num_neighbors=cfg["k"], derivative_indices=cfg["deriv"], radius=cfg["radius"], regularize_lstsq=cfg["reg"])
    idx, w = mod.get_non_uniform_fd_weights(p, **kw)
    der = mod.non_uniform_fd(p, v, **kw)
    der.backward(torch.from_numpy(g).to(dtype))
    return idx.numpy(), w.detach().numpy(), der.detach().numpy(), v.grad.numpy()


def record(name, cfg, mod):
    points, values, g = nr.case_inputs(cfg)
    ex = nr.excluded(points, cfg["k"], cfg["radius"])
    inc = ~ex
    assert ex.mean() <= nr.MAX_EXCLUDED, (name, int(ex.sum()))
    g[:, ex] = 0.0
    idx, w, der, grad = run_reference(mod, cfg, points, values, g, torch.float64)
    # the helper's closed form is what the reference computes
    hidx, _, _, hw = nr.closed_form(points, cfg["k"], cfg["deriv"], cfg["radius"], nr.LAMBDA if cfg["reg"] else 0.0)
    assert nr.same_sets(hidx[inc], idx[inc]).all(), name
    closed = nr.rel_l2(nr.match_by_index(hidx[inc], hw[inc], idx[inc]), w[inc])
    assert closed <= 1e-10, (name, closed)
    idx32, w32, der32, grad32 = run_reference(mod, cfg, points, values, g, torch.float32)
    same = nr.same_sets(idx32, idx) & inc
    out = {"points": points, "values": values, "g": g, "ref:indices": idx.astype(np.int32), "ref:derivatives": der,
           "ref:grad:values": grad, "err:model": np.float64(nr.model_error(w, idx, values[None], inc)),
           "err:weights": np.float64(nr.rel_l2(nr.match_by_index(idx32[same], w32[same], idx[same]), w[same])),
           "err:derivatives": np.float64(nr.rel_l2(der32[:, inc], der[:, inc])),
           "err:grad:values": np.float64(nr.rel_l2(grad32, grad))}
    out["ref:weights"] = w.astype(np.float32) if w.nbytes > 150_000 else w
    np.savez_compressed(nr.fixture_path(name), **out)
    size = os.path.getsize(nr.fixture_path(name))
    assert size < 400_000, (name, size)
    print(f"{name}: excluded {int(ex.sum())} of {len(ex)}, closed form {closed:.1e}, fp32 reference: weights "
          f"{float(out['err:weights']):.1e} derivatives {float(out['err:derivatives']):.1e} grad "
          f"{float(out['err:grad:values']):.1e}, model {float(out['err:model']):.1e}, {size} bytes")


if __name__ == "__main__":
    module = fr.load_reference_differentiation()
    for case_name in sorted(nr.CASES):
        record(case_name, nr.CASES[case_name], module)
