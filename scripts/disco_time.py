"""Equidistant discrete-continuous convolutions and one LocalNOBlocks layer on one MI355X, for manual use (no test runs
this):

    python scripts/disco_time.py [--iters 20] [--out profiles/disco.txt]

B = 8, C = 64, default kernel shape [2, 4]: 256 x 256 -> 256 x 256 (3 x 3 support, stride 1: the matrix-core route) and
256 x 256 -> 128 x 128 (5 x 5 support, stride 2: the vector-ALU route).  Forward and forward + backward of the engine's
layer beside the reference's formula as a torch op chain on the same GPU (einsum that materialises the kernel, then
F.conv2d: ATen / MIOpen launches; the parent of this change has nothing to compare with).  The dense forward also
beside its priced matrix floor (2 B H W C_in C_out taps flops at the fp32 matrix peak of 157 TFLOP/s: arithmetic, not
a measurement).  Then one default LocalNOBlocks layer (64 channels, n_modes (64, 64), 256 x 256): the engine block
beside the same module with its local integral branch computed by the torch op chain.  Events around the whole loop
after a warm-up."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuraloperator_amd import EquidistantDiscreteContinuousConv2d, LocalNOBlocks  # noqa: E402

B, C, N = 8, 64, 256
MATRIX_PEAK = 157e12                                 # fp32 matrix flop/s


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
    kernel = torch.einsum("kxy,ogk->ogxy", m.get_local_filter_matrix(), m.weight)
    pad = ((m.psi_local_h + 1) // 2 - 1, (m.psi_local_w + 1) // 2 - 1)
    return F.conv2d(m.q_weight * x, kernel, m.bias, stride=[m.scale_h, m.scale_w], dilation=1, padding=pad,
                    groups=m.groups)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, C, N, N, generator=g).to(dev).requires_grad_(True)
    lines = [f"B={B} C={C} kernel_shape=[2, 4], fp32; us per call",
             f"{'layer':>16s} {'step':>10s} {'engine':>10s} {'torch':>10s} {'floor':>10s}"]
    for tag, out in (("256->256 3x3", N), ("256->128 5x5", N // 2)):
        m = EquidistantDiscreteContinuousConv2d(C, C, (N, N), (out, out), [2, 4]).to(dev)
        assert m.on_engine(x)
        gout = torch.randn(B, C, out, out, generator=g).to(dev)
        err = float((m(x) - torch_formula(m, x)).norm() / torch_formula(m, x).norm())
        assert err < 1e-5, err

        def step(fn):
            x.grad = None
            m.zero_grad(set_to_none=True)
            fn().backward(gout)

        flops = 2.0 * B * out * out * C * C * m.psi_local_h * m.psi_local_w
        floor = flops / MATRIX_PEAK * 1e6
        with torch.no_grad():
            fwd = (timed(lambda: m(x), args.iters), timed(lambda: torch_formula(m, x), args.iters), floor)
        both = (timed(lambda: step(lambda: m(x)), args.iters),
                timed(lambda: step(lambda: torch_formula(m, x)), max(args.iters // 4, 2)), 3 * floor)
        for name, (t_eng, t_ref, t_floor) in (("fwd", fwd), ("fwd+bwd", both)):
            lines.append(f"{tag:>16s} {name:>10s} {t_eng:10.1f} {t_ref:10.1f} {t_floor:10.1f}")
            print(lines[-1], flush=True)

    blocks = LocalNOBlocks(C, C, (64, 64), (N, N), n_layers=2).to(dev)
    gout = torch.randn(B, C, N, N, generator=g).to(dev)
    disco = blocks.local_convs[0]
    engine_forward = type(disco).forward

    def block_step():
        x.grad = None
        blocks.zero_grad(set_to_none=True)
        blocks(x, 0).backward(gout)

    t_eng_f, t_eng = timed(lambda: blocks(x, 0).detach(), args.iters), timed(block_step, args.iters)
    type(disco).forward = torch_formula                      # the same block, local integral branch through ATen / MIOpen
    try:
        t_ref_f, t_ref = timed(lambda: blocks(x, 0).detach(), args.iters), timed(block_step, max(args.iters // 4, 2))
    finally:
        type(disco).forward = engine_forward
    lines.append(f"{'LocalNOBlocks':>16s} {'fwd':>10s} {t_eng_f:10.1f} {t_ref_f:10.1f} {'-':>10s}")
    lines.append(f"{'LocalNOBlocks':>16s} {'fwd+bwd':>10s} {t_eng:10.1f} {t_ref:10.1f} {'-':>10s}")
    lines.append("LocalNOBlocks: one default layer, 64 channels, n_modes (64, 64), 256 x 256; 'torch' = the same engine "
                 "block with only its local integral branch as the torch op chain")
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
