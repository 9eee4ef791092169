"""AttentionKernelIntegral on one MI355X, for manual use (no test runs this):

    python scripts/attention_time.py [--iters 30] [--repeats 5] [--out profiles/attention.txt]

Two shapes of the layer, B = 4, C = 128 in and out:
    N = 128 x 128, H = 4, D = 32, 2-d rotary embedding
    N =  64 x  64, H = 2, D = 64, no rotary embedding
Forward and forward + backward of the layer on the engine route beside the same layer on the torch route (the
reference's formula as a chain of torch calls) on the same GPU, alternating the two, `repeats` windows of `iters` calls
each between device events after a warm-up: the median and the range of the windows are printed.  Peak allocated memory
of one forward + backward step of each route above what is allocated before the step.  The priced floor is arithmetic,
not a measurement: the accesses of T = B N H D floats the fused passes need (FLOOR_ACCESSES: four forward, eight more
backward; the projections are not priced) at the copy rate this script measures on the box with a device-to-device
copy of 256 MB.

Each shape is measured in a process of its own under a time limit (--one runs a single shape): a fault or a hang in one
ends that step and nothing after it is started."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, C = 4, 128
SHAPES = {"n16384_h4_d32_rot2": (128 * 128, 4, 32, True), "n4096_h2_d64_plain": (64 * 64, 2, 64, False)}
# T-sized accesses of the fused passes: forward reads k, v, q and writes u; backward reads g_u and q (g_dots), g_u again
# (g_q), k and v, and writes g_q, g_k, g_v
FLOOR_ACCESSES = {"fwd": 4, "fwd+bwd": 4 + 8}
STEP_LIMIT = 300


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us


def alternate(fns, iters, repeats, warmup=3):
    """`repeats` windows of each function, the functions taking turns: [(median, low, high)] in us"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            times[i].append(window(fn, iters))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def copy_rate():
    """bytes per second of a device-to-device copy of 256 MB (read + write counted)"""
    src = torch.empty(64 << 20, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    us = alternate([lambda: dst.copy_(src)], 20, 3)[0][0]
    return 2 * src.numel() * 4 / (us * 1e-6)


def peak_of(step):
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def one(tag, iters, repeats):
    from neuraloperator_amd import AttentionKernelIntegral, RotaryEmbedding2D, attention
    n, heads, d, rotary = SHAPES[tag]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = AttentionKernelIntegral(C, C, heads, d).to(dev)
    emb = RotaryEmbedding2D(d // 2).to(dev) if rotary else None
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, n, C, generator=g).to(dev).requires_grad_(True)
    pos = torch.rand(B, n, 2, generator=g).to(dev)
    gout = torch.randn(B, n, C, generator=g).to(dev)
    assert m.on_engine(x, pos, positional_embedding_module=emb)

    def call(route):
        with attention.route(route):
            return m(x, pos, positional_embedding_module=emb)

    def step(route):
        x.grad = None
        m.zero_grad(set_to_none=True)
        call(route).backward(gout)

    with torch.no_grad():
        want = call("torch")
        err = float((call("engine") - want).norm() / want.norm())
    assert err < 1e-5, err
    rate = copy_rate()
    T = B * n * heads * d * 4
    with torch.no_grad():
        fwd = alternate([lambda: call("engine"), lambda: call("torch")], iters, repeats)
    both = alternate([lambda: step("engine"), lambda: step("torch")], iters, repeats)
    mem = [peak_of(lambda: step("engine")), peak_of(lambda: step("torch"))]
    for name, (eng, ref) in (("fwd", fwd), ("fwd+bwd", both)):
        floor = FLOOR_ACCESSES[name] * T / rate * 1e6
        print(f"{tag:>20s} {name:>8s} {eng[0]:9.1f} [{eng[1]:.1f}, {eng[2]:.1f}] {ref[0]:9.1f} [{ref[1]:.1f}, {ref[2]:.1f}] "
              f"{floor:8.1f} {ref[0] / eng[0]:8.2f}", flush=True)
    print(f"{tag:>20s} peak MiB of a fwd+bwd step: engine {mem[0]:.0f}, torch {mem[1]:.0f}; T = {T / 2 ** 20:.0f} MiB; "
          f"copy rate {rate / 1e12:.2f} TB/s; engine against torch forward rel-L2 {err:.1e}; {repeats} windows of {iters}",
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="measure this shape alone, in this process")
    args = ap.parse_args()
    if args.one is not None:
        return one(args.one, args.iters, args.repeats)
    lines = [f"B={B} C={C} fp32, the layer with its four projections; us per call: median [min, max] of the windows",
             f"{'shape':>20s} {'step':>8s} {'engine':>9s} {'':>16s} {'torch':>9s} {'':>16s} {'floor':>8s} {'torch/eng':>8s}"]
    ok = True
    for tag in SHAPES:                                       # a fresh process per shape, each under its own limit
        r = subprocess.run(["timeout", "-k", "10", str(STEP_LIMIT), sys.executable, os.path.abspath(__file__), "--one", tag,
                            "--iters", str(args.iters), "--repeats", str(args.repeats)], capture_output=True, text=True)
        lines += [ln for ln in r.stdout.splitlines() if ln.strip()]
        if r.returncode != 0:
            lines.append(f"{tag}: exit status {r.returncode}; nothing further was started\n" + r.stderr[-2000:])
            ok = False
            break
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
