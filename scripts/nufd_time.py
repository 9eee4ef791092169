"""Point-cloud finite differences on one MI355X, for manual use (no test runs this):

    python scripts/nufd_time.py [--iters 20] [--repeats 5] [--out profiles/nufd.txt]

Two clouds of uniformly random points, every coordinate differentiated, B = 8 fields:
    N =  16 384, d = 2, k =  9
    N = 100 000, d = 3, k = 16
The stencil build (neighbour search, weights, transpose) and one apply + backward step of NonUniformFD on the engine
route beside the same class on the torch route (the reference's formula as a chain of torch calls: cdist, topk, lstsq,
gather + einsum) on the same GPU, alternating the two, `repeats` windows between device events after a warm-up: the
median and the range of the windows are printed.  A build window is ONE build (the torch build of the large cloud forms
a 40 GB distance matrix); a step window is `iters` steps.  Peak allocated memory of one build and of one step of each
route above what is allocated before it.  Where the torch chain fails (out of memory, an unsupported solve) the line
says so and the engine's figures stand alone.

Each cloud is measured in a process of its own under a time limit (--one runs a single cloud): a fault or a hang in one
ends that step and nothing after it is started."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B = 8
SHAPES = {"n16384_d2_k9": (16384, 2, 9), "n100000_d3_k16": (100000, 3, 16)}
STEP_LIMIT = 420


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us


def alternate(fns, iters, repeats, warmup=2):
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


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    keep = fn()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    del keep
    return peak


def fmt(t):
    return "failed".rjust(34) if t is None else f"{t[0]:12.1f} [{t[1]:.1f}, {t[2]:.1f}]".rjust(34)


def one(tag, iters, repeats):
    from neuraloperator_amd import NonUniformFD, differentiation
    n, d, k = SHAPES[tag]
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    points = torch.rand(n, d, generator=gen).to(dev)
    values = torch.sin(3.0 * torch.rand(B, 1, d, generator=gen).to(dev) + 3.0 * points).sum(-1).requires_grad_(True)
    gout = torch.randn(d, B, n, generator=gen).to(dev)
    deriv = list(range(d))

    def build(route):
        with differentiation.route(route):
            return NonUniformFD(points, k, deriv)

    fd = {"engine": build("engine")}
    why = ""
    try:
        fd["torch"] = build("torch")
        torch.cuda.synchronize()
    except RuntimeError as e:                                # out of memory, a solve the library lacks
        why = f"; the torch build failed: {str(e).splitlines()[0][:160]}"
        torch.cuda.empty_cache()
    routes = list(fd)

    def step(route):
        values.grad = None
        with differentiation.route(route):
            fd[route](values).backward(gout)

    err = ""
    if "torch" in fd:
        with torch.no_grad():
            want, got = fd["torch"](values), fd["engine"](values)
        err = f"; engine against torch derivatives rel-L2 {float((got - want).norm() / want.norm()):.1e}"
    flagged = int(fd["engine"].ill_posed().numel())
    bt = dict(zip(routes, alternate([lambda r=r: build(r) for r in routes], 1, repeats, warmup=1)))
    st = dict(zip(routes, alternate([lambda r=r: step(r) for r in routes], iters, repeats)))
    mem_b = {r: peak_of(lambda r=r: build(r)) for r in routes}
    mem_s = {r: peak_of(lambda r=r: step(r)) for r in routes}
    for name, t, mem in (("build", bt, mem_b), ("fwd+bwd", st, mem_s)):
        ratio = f"{t['torch'][0] / t['engine'][0]:9.2f}" if "torch" in t else "        -"
        peak_t = f"{mem['torch']:10.1f}" if "torch" in mem else "         -"
        print(f"{tag:>16s} {name:>8s} {fmt(t['engine'])} {fmt(t.get('torch'))} {ratio} {mem['engine']:10.1f} {peak_t}", flush=True)
    print(f"{tag:>16s} N k = {n * k * 4 / 2 ** 20:.1f} MiB of fp32, N^2 = {n * n * 4 / 2 ** 20:.0f} MiB; {flagged} ill-posed points"
          f"{err}{why}; {repeats} windows", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="measure this cloud alone, in this process")
    args = ap.parse_args()
    if args.one is not None:
        return one(args.one, args.iters, args.repeats)
    lines = [f"B={B} fields, fp32, every coordinate differentiated; us per build / per step: median [min, max] of the "
             "windows; peak MiB above what was allocated before",
             f"{'cloud':>16s} {'':>8s} {'engine':>34s} {'torch':>34s} {'torch/eng':>9s} {'peak eng':>10s} {'peak torch':>10s}"]
    ok = True
    for tag in SHAPES:                                       # a fresh process per cloud, each under its own limit
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
