"""spectral_projection_divergence_free on one MI355X, for manual use (no test runs this):

    python scripts/spectral_projection_time.py [--iters 30] [--repeats 5] [--out profiles/spectral_projection.txt]

Two shapes, fp32:
    B = 8,  256 x  256, full modes                          forward
    B = 8, 1024 x 1024, constraint_modes = (128, 128)       forward and forward + backward
The function on its engine route beside its torch route (the same multiplier between torch's rfftn / irfftn) on the
same GPU, alternating the two, `repeats` windows of `iters` calls each between device events after a warm-up: the
median and the range of the windows are printed.  sc_helmholtz_project alone, in place on the kept block, is timed the
same way.  The priced floor is arithmetic, not a measurement: the bytes the three steps of the engine route have to move
-- the forward transform reads the field and writes the kept block, the projector reads and writes the block, the
inverse transform reads the block and writes the field; twice that for forward + backward -- at the copy rate this
script measures on the box with a device-to-device copy of 256 MB.

The verdict line says what "auto" should do: it takes the engine only if the engine's median is below the torch
route's at every row by more than the spread of the windows (the larger of the two ranges).

Each shape is measured in a process of its own under a time limit (--one runs a single shape): a fault or a hang in one
ends that step and nothing after it is started."""
import argparse
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# tag -> (B, H, W, constraint_modes, domain_size, steps)
SHAPES = {"b8_256x256_full": (8, 256, 256, (256, 256), 1.0, ("fwd",)),
          "b8_1024x1024_m128": (8, 1024, 1024, (128, 128), 1.0, ("fwd", "fwd+bwd"))}
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


def one(tag, iters, repeats):
    from neuraloperator_amd import _lib, engine, spectral_projection as sp
    b, h, w, modes, domain, steps = SHAPES[tag]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1)
    u = torch.randn(b, 2, h, w, generator=g).to(dev).requires_grad_(True)
    gout = torch.randn(b, 2, h, w, generator=g).to(dev)

    def call(route):
        with sp.route(route):
            return sp.spectral_projection_divergence_free(u, domain, modes)

    def step(route):
        u.grad = None
        call(route).backward(gout)

    with sp.route("engine"):
        assert sp.on_engine(u, domain, modes)
    with torch.no_grad():
        want = call("torch")
        err = float((call("engine") - want).norm() / want.norm())
    assert err < 1e-5, err
    key = ("reference", h, w, float(domain), float(domain), min(modes[0], h), min(modes[1], w))
    tabs = engine.get_helmholtz_tables(dev, key, None)          # cached by the calls above
    rate = copy_rate()
    field, block = b * 2 * h * w * 4, b * 2 * tabs.kept[0] * tabs.kept[1] * 8
    floor = (2 * field + 4 * block) / rate * 1e6
    rows = []
    if "fwd" in steps:
        with torch.no_grad():
            rows.append(("fwd", floor) + tuple(alternate([lambda: call("engine"), lambda: call("torch")], iters, repeats)))
    if "fwd+bwd" in steps:
        rows.append(("fwd+bwd", 2 * floor) + tuple(alternate([lambda: step("engine"), lambda: step("torch")], iters,
                                                             repeats)))
    faster = True
    for name, fl, eng, ref in rows:
        spread = max(eng[2] - eng[1], ref[2] - ref[1])
        faster = faster and eng[0] + spread < ref[0]
        print(f"{tag:>20s} {name:>8s} {eng[0]:9.1f} [{eng[1]:.1f}, {eng[2]:.1f}] {ref[0]:9.1f} [{ref[1]:.1f}, {ref[2]:.1f}] "
              f"{fl:8.1f} {ref[0] / eng[0]:8.2f}", flush=True)
    xh = torch.randn(b, 2, *tabs.kept, 2, device=dev)
    moved = torch.empty(2 * xh.numel(), dtype=torch.float32, device=dev)      # copy_ of one half onto the other
    half = moved.numel() // 2
    lib, modes = _lib.get_lib(), tabs.kept[0] * tabs.kept[1]
    project = lambda: lib.helmholtz_project(xh.data_ptr(), xh.data_ptr(), kept=tabs.kept, groups=b, sel=tabs.sel,
                                            eps=tabs.eps, tabs=tabs.ptrs, y_group_stride=2 * modes, y_comp_stride=modes,
                                            stream=torch.cuda.current_stream().cuda_stream)
    ker, cp = alternate([project, lambda: moved[:half].copy_(moved[half:])], iters, repeats)
    print(f"{tag:>20s} kept {tabs.kept[0]} x {tabs.kept[1]}: sc_helmholtz_project in place {ker[0]:.1f} [{ker[1]:.1f}, "
          f"{ker[2]:.1f}] us ({2 * block / ker[0] / 1e6:.2f} TB/s), copy_ of the same {2 * block / 2 ** 20:.0f} MiB moved "
          f"{cp[0]:.1f} [{cp[1]:.1f}, {cp[2]:.1f}] us; copy rate {rate / 1e12:.2f} TB/s; engine against torch forward rel-L2 "
          f"{err:.1e}; {repeats} windows of {iters}; engine faster than torch by more than the spread: "
          f"{'yes' if faster else 'no'}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one", default=None, help="measure this shape alone, in this process")
    args = ap.parse_args()
    if args.one is not None:
        return one(args.one, args.iters, args.repeats)
    lines = ["spectral_projection_divergence_free, fp32 (B, 2, H, W); us per call: median [min, max] of the windows",
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
    if ok:
        every = all("more than the spread: yes" in ln for ln in lines if "more than the spread" in ln)
        lines.append(f'verdict: "auto" {"takes the engine" if every else "stays on the torch route; the engine route is opt-in"}')
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
