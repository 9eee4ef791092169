"""Time the 2-d skip-path resample of the spatially decomposed layer at one rank (SpatialParallelSpectralConv.transform,
the sc_bicubic_rows kernels) against F.interpolate(bicubic, align_corners=True), forward + backward, on the same
tensor in the same process; also the device copy rate of the box (a device-to-device copy of the same bytes).
Prints one JSON line per case.  ``--iters N --warmup W``."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    from neuraloperator_amd.mpu import SpatialParallelSpectralConv
    dev = torch.device("cuda:0")
    B, C = 4, 64
    for grid, out in (((1024, 1024), (2048, 2048)), ((2048, 2048), (1024, 1024))):
        sp = SpatialParallelSpectralConv(C, C, (16, 16)).to(dev)
        x = torch.randn(B, C, *grid, device=dev, requires_grad=True)
        g = torch.randn(B, C, *out, device=dev)

        def ours():
            x.grad = None
            sp.transform(x, output_shape=out).backward(g)

        def aten():
            x.grad = None
            F.interpolate(x, size=out, mode="bicubic", align_corners=True).backward(g)

        with torch.no_grad():
            y0 = sp.transform(x, output_shape=out)
            y1 = F.interpolate(x, size=out, mode="bicubic", align_corners=True)
            err = float((y0 - y1).double().norm() / y1.double().norm())
        t_ours, t_aten = [], []
        for _ in range(2):                                   # alternate the two
            t_ours.append(_time(ours, a.warmup, a.iters))
            t_aten.append(_time(aten, a.warmup, a.iters))
        src = torch.empty(B * C * max(grid[0] * grid[1], out[0] * out[1]), device=dev)
        dst = torch.empty_like(src)
        t_copy = _time(lambda: dst.copy_(src), a.warmup, a.iters)
        nbytes = 4 * B * C * (grid[0] * grid[1] + out[0] * out[1])   # in + out per pass
        print(json.dumps(dict(case=f"{grid[0]}x{grid[1]}->{out[0]}x{out[1]}", B=B, C=C, fwd_bwd_ms=min(t_ours),
                              aten_fwd_bwd_ms=min(t_aten), runs_ms=dict(ours=t_ours, aten=t_aten),
                              rel_l2_vs_aten=err, bytes_per_pass=nbytes,
                              copy_GBps=2 * src.numel() * 4 / t_copy / 1e6)), flush=True)


if __name__ == "__main__":
    main()
