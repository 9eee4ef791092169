"""Time the complex32 wire kernels (sc_kernels_wire.h) at the per-rank shapes of BASELINE configs[3] on 8 ranks.

configs[3]: FNO3d 128^3, n_modes (32, 32, 32) -> kept block 32 x 32 x 17, hidden 32, one sample per rank; a rank owns 4 of
the 32 first-dim mode rows.  The four calls of one exchange pair:

    pack_out     xhat (1, 32, 32, 32, 17) c64 -> wire (8, 1, 32, 4, 32, 17) c32     (placed rows)
    unpack_out   wire (8, 1, 32, 4, ...) c32 -> (8, 32, 4, 32, 17) c64            (plain conversion)
    pack_back    yhat (8, 32, 4, 32, 17) c64 -> wire (1, 8, 32, 4, ...) c32        (plain conversion)
    unpack_back  wire (8, 1, 32, 4, ...) c32 -> (1, 32, 32, 32, 17) c64            (row window)

Per call: device-event time over a loop of launches (after a warm-up), microseconds per call and GB/s of bytes read +
written.  For scale, the same box's device-to-device copy rate: torch copy_ of an fp32 buffer of the complex64 side's size
(4.46 MB, the same cache regime) and of 512 MB (HBM).  One JSON line on stdout; --out writes it to a file as well.
The multi-GPU exchange itself is not timed here."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters           # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from neuraloperator_amd import engine

    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    P, rows, k1, C, rest = 8, 4, 32, 32, (32, 17)
    m = rows * rest[0] * rest[1]
    xhat = torch.randn(1, C, k1, *rest, dtype=torch.complex64, device=dev)
    yloc = torch.randn(P, C, rows, *rest, dtype=torch.complex64, device=dev)
    wire = engine.wire_pack_c32(xhat, P, rows, 0)
    c64 = P * C * m * 8                                # bytes of the complex64 side of every call
    c32 = c64 // 2
    calls = {
        "pack_out": lambda: engine.wire_pack_c32(xhat, P, rows, 0),
        "unpack_out": lambda: engine.wire_unpack_c32(wire.view(1, P, C, rows, *rest), rows, 0),
        "pack_back": lambda: engine.wire_pack_c32(yloc, 1, rows, 0),
        "unpack_back": lambda: engine.wire_unpack_c32(wire, k1, 0),
    }
    res = {"shape": "configs[3] per rank of 8: xhat (1, 32, 32, 32, 17), 4 rows per rank", "bytes_c64": c64,
           "bytes_c32": c32}
    for name, fn in calls.items():
        ts = sorted(_time(fn, args.iters, args.warmup) for _ in range(args.repeats))
        us = ts[len(ts) // 2]
        res[name] = {"us": round(us, 2), "us_min": round(ts[0], 2), "us_max": round(ts[-1], 2),
                     "GBps": round((c64 + c32) / us / 1e3, 1)}
    for label, nbytes in (("copy_4p46MB", c64), ("copy_512MB", 512 << 20)):
        src = torch.empty(nbytes // 4, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        it = args.iters if nbytes < (64 << 20) else 50
        ts = sorted(_time(lambda: dst.copy_(src), it, 10) for _ in range(args.repeats))
        us = ts[len(ts) // 2]
        res[label] = {"us": round(us, 2), "GBps": round(2 * nbytes / us / 1e3, 1)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
