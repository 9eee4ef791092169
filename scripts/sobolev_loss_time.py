"""H1Loss / LpLoss(p=2) forward + backward on one MI355X, for manual use (no test runs this):

    python scripts/sobolev_loss_time.py [--iters 200] [--out profiles/sobolev_loss.txt]

Three columns per shape: this code; the same formulas as the torch operator chain the reference issues (rolls,
differences, flattens, squared sums, roots, a divide, a sum, and autograd's mirror image), written out here; and a
device-to-device copy of the bytes the fused passes must move -- 2 reads forward, 2 reads + 1 write backward = 5 fields,
timed as copy_ of 2.5 fields (a copy reads and writes each byte once).  Events around the whole loop after a warm-up;
periodic axes."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuraloperator_amd import H1Loss, LpLoss  # noqa: E402

SHAPES = [(32, 1, 256, 256), (8, 1, 128, 128, 128), (4, 1, 1024, 1024)]


def chain_h1(x, y, d, eps=1e-8):
    q = [1.0 / x.size(-j) for j in range(d, 0, -1)]
    fx, fy = [x], [y]
    for a in range(d):
        for src, dst in ((x, fx), (y, fy)):
            dst.append((torch.roll(src, -1, dims=a - d) - torch.roll(src, 1, dims=a - d)) / (2.0 * q[a]))
    diff = torch.sum((torch.flatten(fx[0], start_dim=-d) - torch.flatten(fy[0], start_dim=-d)) ** 2, dim=-1)
    ynorm = torch.sum(torch.flatten(fy[0], start_dim=-d) ** 2, dim=-1)
    for j in range(1, d + 1):
        diff = diff + torch.sum((torch.flatten(fx[j], start_dim=-d) - torch.flatten(fy[j], start_dim=-d)) ** 2, dim=-1)
        ynorm = ynorm + torch.sum(torch.flatten(fy[j], start_dim=-d) ** 2, dim=-1)
    return torch.sum((diff ** 0.5) / (ynorm ** 0.5 + eps)).squeeze()


def chain_lp2(x, y, d, eps=1e-8):
    diff = torch.sum((torch.flatten(x, start_dim=-d) - torch.flatten(y, start_dim=-d)) ** 2, dim=-1)
    ynorm = torch.sum(torch.flatten(y, start_dim=-d) ** 2, dim=-1)
    return torch.sum((diff ** 0.5) / (ynorm ** 0.5 + eps)).squeeze()


def timed(fn, iters, warmup=20):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"{'loss':6s} {'shape':>18s} {'engine us':>10s} {'torch chain us':>15s} {'copy us':>8s} "
             f"{'engine/copy':>11s} {'chain/engine':>12s}"]
    for shape in SHAPES:
        d = len(shape) - 2
        g = torch.Generator().manual_seed(1)
        x = torch.randn(*shape, generator=g).to(dev).requires_grad_(True)
        y = torch.randn(*shape, generator=g).to(dev)
        n = x.numel()
        src, dst = torch.empty(n * 5 // 2, device=dev), torch.empty(n * 5 // 2, device=dev)
        t_copy = timed(lambda: dst.copy_(src), args.iters)
        for name, ours, chain in (("H1", H1Loss(d=d), chain_h1), ("L2", LpLoss(d=d, p=2), chain_lp2)):
            def step(f):
                x.grad = None
                f().backward()
            t_eng = timed(lambda: step(lambda: ours(x, y)), args.iters)
            t_ref = timed(lambda: step(lambda: chain(x, y, d)), args.iters)
            lines.append(f"{name:6s} {'x'.join(map(str, shape)):>18s} {t_eng:10.1f} {t_ref:15.1f} {t_copy:8.1f} "
                         f"{t_eng / t_copy:11.2f} {t_ref / t_eng:12.2f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
