"""FiniteDifferenceConvolution on one MI355X, for manual use (no test runs this):

    python scripts/fdconv_time.py [--iters 20] [--out profiles/fdconv.txt]

B = 8, C = 64, 256 x 256, k = 3, periodic -- dense (groups = 1: the matrix-core route) and depthwise (groups = C: the
vector-ALU route).  Forward and forward + backward of the engine's layer beside the reference's formula in torch on the
same GPU (the padded k^d convolution, the 1 x 1 convolution of the summed kernel, the subtraction and the division:
ATen / MIOpen launches, which is all the parent of this change has) and beside a device-to-device copy of the step's
algorithmic bytes (x and y once forward; x, gout, gx once more backward).  Events around the whole loop after a
warm-up."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuraloperator_amd import FiniteDifferenceConvolution  # noqa: E402

B, C, H, W, K, GRID_WIDTH = 8, 64, 256, 256, 3, 1.0 / 256


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


def copy_us(nbytes, iters):
    n = max(int(nbytes) // 8, 1)                    # a copy reads and writes every byte once
    src, dst = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
    return timed(lambda: dst.copy_(src), iters)


def torch_formula(m, x, h):
    spatial = tuple(range(2, 2 + m.n_dim))
    centre = m.conv_function(x, m.weight.sum(dim=spatial, keepdim=True), groups=m.groups)
    return (m.conv(x) - centre) / h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, C, H, W, generator=g).to(dev).requires_grad_(True)
    gout = torch.randn(B, C, H, W, generator=g).to(dev)
    tensor_bytes = 4 * B * C * H * W
    lines = [f"B={B} C={C} {H}x{W} k={K} periodic, fp32; us per call",
             f"{'layer':>10s} {'step':>10s} {'engine':>10s} {'torch':>10s} {'copy':>10s}"]
    for tag, groups in (("dense", 1), ("depthwise", C)):
        m = FiniteDifferenceConvolution(C, C, 2, kernel_size=K, groups=groups).to(dev)
        assert m.on_engine(x, GRID_WIDTH)

        def step(fn):
            x.grad = None
            m.zero_grad(set_to_none=True)
            fn().backward(gout)

        with torch.no_grad():
            fwd = (timed(lambda: m(x, GRID_WIDTH), args.iters), timed(lambda: torch_formula(m, x, GRID_WIDTH), args.iters),
                   copy_us(2 * tensor_bytes, args.iters))
        both = (timed(lambda: step(lambda: m(x, GRID_WIDTH)), args.iters),
                timed(lambda: step(lambda: torch_formula(m, x, GRID_WIDTH)), max(args.iters // 4, 2)),
                copy_us(5 * tensor_bytes, args.iters))
        for name, (t_eng, t_ref, t_copy) in (("fwd", fwd), ("fwd+bwd", both)):
            lines.append(f"{tag:>10s} {name:>10s} {t_eng:10.1f} {t_ref:10.1f} {t_copy:10.1f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
