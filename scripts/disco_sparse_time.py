"""Discrete-continuous convolutions on point clouds on one MI355X, for manual use (no test runs this):

    python scripts/disco_sparse_time.py [--iters 20] [--out profiles/disco_sparse.txt]

B = 8, C = 64, kernel shape [2, 4], default cut-off, uniform random clouds of the unit square: 16 384 -> 16 384 points and
16 384 -> 4 096 points.  Forward and forward + backward of the engine's layer beside the reference's formula as a torch
op chain on the same GPU (a sparse COO matrix per call, a transposed copy of the input, torch.sparse.mm, einsum; the
parent of this change has nothing to compare with), and beside the priced floor: K x the activation bytes for Z written
and read once each at 8 TB/s plus 2 B n_out C_out C_in K flops at the fp32 matrix peak of 157 TFLOP/s (arithmetic, not a
measurement; forward + backward is priced at three times the forward).  Events around the whole loop after a warm-up.

Each shape is measured in a process of its own under a time limit (--one runs a single shape): a fault or a hang in one
ends that step and nothing after it is started."""
import argparse
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, C, N_IN = 8, 64, 16384
SHAPES = (16384, 4096)
MATRIX_PEAK, HBM = 157e12, 8e12                      # fp32 matrix flop/s, bytes/s
# seconds for one shape.  Building Psi on the host takes about 30 s at 16 384 x 16 384 points and 8 s at 16 384 x 4 096
# (measured on a 16-thread host); the check against the torch chain and the timed loops are a few seconds more
STEP_LIMIT = 240


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us


def torch_formula(m, x):
    x = m.quadrature_weights * x
    psi = m.get_local_filter_matrix()
    b, c, _ = x.shape
    x = x.reshape(b * c, m.n_in).permute(1, 0).contiguous()
    x = torch.sparse.mm(psi, x)
    x = x.permute(1, 0).reshape(b, m.groups, m.groupsize, m.kernel_size, m.n_out)
    out = torch.einsum("bgckx,gock->bgox", x, m.weight.reshape(m.groups, -1, m.weight.shape[1], m.weight.shape[2]))
    return out.reshape(b, -1, m.n_out) + m.bias.reshape(1, -1, 1)


def one(n_out, iters):
    from neuraloperator_amd import DiscreteContinuousConv2d, _lib, engine
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    grid_in, grid_out = torch.rand(2, N_IN, generator=g), torch.rand(2, n_out, generator=g)
    m = DiscreteContinuousConv2d(C, C, grid_in, grid_out, [2, 4], quadrature_weights=torch.full((N_IN,), 1.0 / N_IN)).to(dev)
    x = torch.randn(B, C, N_IN, generator=g).to(dev).requires_grad_(True)
    gout = torch.randn(B, C, n_out, generator=g).to(dev)
    assert m.on_engine(x)
    path = _lib.get_lib().dsparse_path(engine.SparseDiscoFn.desc(x, m.weight, m.n_out, m.csr_vals.numel(), m.groups))
    want = torch_formula(m, x)
    err = float((m(x) - want).norm() / want.norm())
    assert err < 1e-5, err

    def step(fn):
        x.grad = None
        m.zero_grad(set_to_none=True)
        fn().backward(gout)

    K = m.kernel_size
    floor = (2.0 * K * B * C * n_out * 4 / HBM + 2.0 * B * n_out * C * C * K / MATRIX_PEAK) * 1e6
    with torch.no_grad():
        fwd = (timed(lambda: m(x), iters), timed(lambda: torch_formula(m, x), iters), floor)
    both = (timed(lambda: step(lambda: m(x)), iters), timed(lambda: step(lambda: torch_formula(m, x)), max(iters // 4, 2)),
            3 * floor)
    tag = f"{N_IN}->{n_out}"
    for name, (t_eng, t_ref, t_floor) in (("fwd", fwd), ("fwd+bwd", both)):
        print(f"{tag:>14s} {name:>8s} {t_eng:10.1f} {t_ref:10.1f} {t_floor:10.1f} {t_ref / t_eng:8.2f} {t_eng / t_floor:8.1f}"
              f"   route {path} nnz {m.psi_vals.numel()} ({m.psi_vals.numel() / (K * n_out):.1f} per row) K {K}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", type=int, default=None, help="measure this n_out alone, in this process")
    args = ap.parse_args()
    if args.one is not None:
        return one(args.one, args.iters)
    lines = [f"B={B} C={C} kernel_shape=[2, 4], default cut-off 2 / (sqrt(n_out) - 1), fp32; us per call",
             f"{'points':>14s} {'step':>8s} {'engine':>10s} {'torch':>10s} {'floor':>10s} {'torch/eng':>8s} {'eng/floor':>8s}"]
    for n_out in SHAPES:                                     # a fresh process per shape, each under its own limit
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--one",
                            str(n_out), "--iters", str(args.iters)], capture_output=True, text=True)
        lines += [ln for ln in r.stdout.splitlines() if ln.strip()]
        if r.returncode != 0:
            lines.append(f"{N_IN}->{n_out}: exit status {r.returncode}; nothing further was started\n" + r.stderr[-2000:])
            break
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)
    return 0 if len(lines) == 2 + 2 * len(SHAPES) else 1


if __name__ == "__main__":
    sys.exit(main())
