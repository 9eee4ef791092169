"""Timing of neuraloperator_amd.FourierDiff on one GPU (no test asserts these numbers):

  * gradient / laplacian, whole operator, against the reference's formula as a torch op chain (full complex fftn, one
    dense (1j K)**order multiplier per derivative, complex ifftn, .real; one chain per term as the reference's dx / dy /
    dz do) on the same GPU in the same process, alternating;
  * sc_spectral_op alone against torch.Tensor.copy_ of the same bytes, (n_src + n_out) * 8 * modes * groups.

    python scripts/fourier_diff_time.py [--out profiles/fourier_diff.txt]
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from neuraloperator_amd import FourierDiff, engine  # noqa: E402


def torch_chain_derivative(u, dim, L, orders):
    """the reference's _compute_multiple_derivatives_{2,3}d for one order tuple, as it runs it"""
    dims = tuple(range(-dim, 0))
    n = u.shape[-dim:]
    uh = torch.fft.fftn(u, dim=dims)
    ks = [torch.fft.fftfreq(n[d], d=L[d] / n[d], device=u.device) * (2 * torch.pi) for d in range(dim)]
    K = torch.meshgrid(*ks, indexing="ij")
    g = None
    for d in range(dim):
        f = (1j * K[d].expand(uh.shape)) ** orders[d]
        g = f if g is None else g * f
    return torch.fft.ifftn(torch.stack([g * uh], dim=0), dim=dims).real[0]


def torch_chain(method, u, dim, L):
    ax = lambda d, o: tuple(o if i == d else 0 for i in range(dim))
    if method == "gradient":
        return torch.stack([torch_chain_derivative(u, dim, L, ax(d, 1)) for d in range(dim)], dim=-dim - 1)
    out = torch_chain_derivative(u, dim, L, ax(0, 2))
    for d in range(1, dim):
        out = out + torch_chain_derivative(u, dim, L, ax(d, 2))
    return out


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def ab(fa, fb, reps, rounds=5):
    """alternating rounds; the median of each side"""
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(fa, reps))
        tb.append(timed(fb, reps))
    return sorted(ta)[rounds // 2], sorted(tb)[rounds // 2], ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fourier_diff_time: needs a GPU (no CPU timing path)")
    dev = torch.device("cuda:0")
    lines = [f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; reps {args.reps} x 5 alternating rounds, "
             "median; host clock around a device synchronise"]
    g = torch.Generator().manual_seed(0)
    for shape, dim in (((8, 64, 256, 256), 2), ((8, 8, 128, 128, 128), 3)):
        L = tuple(1.0 + 0.25 * d for d in range(dim))
        u = torch.randn(*shape, generator=g).to(dev)
        fd = FourierDiff(dim, L=L)
        for method in ("gradient", "laplacian"):
            fe = lambda: getattr(fd, method)(u)
            ft = lambda: torch_chain(method, u, dim, L)
            a, b = fe(), ft()
            err = float((a - b).norm() / b.norm())
            for _ in range(3):
                fe(), ft()
            te, tt, re_, rt = ab(fe, ft, args.reps)
            lines.append(f"{method:9s} {'x'.join(map(str, shape)):>18s}: engine {te * 1e3:8.3f} ms  torch chain "
                         f"{tt * 1e3:8.3f} ms  ratio {tt / te:5.2f}x  rel diff {err:.1e}  (rounds engine "
                         f"{[round(v * 1e3, 3) for v in re_]} torch {[round(v * 1e3, 3) for v in rt]})")
            del a, b
        # the multiplier pass alone against a copy of the same bytes
        spatial = shape[-dim:]
        kept = tuple(spatial[:-1]) + (spatial[-1] // 2 + 1,)
        groups = math.prod(shape[:-dim])
        for method, n_out, orders in (("gradient", dim, 1), ("laplacian", 1, 2)):
            ax = lambda d, o: tuple(o if i == d else 0 for i in range(dim))
            terms = [(0, d if method == "gradient" else 0, 1.0, ax(d, orders)) for d in range(dim)]
            xh = torch.randn(groups, 1, *kept, dtype=torch.complex64, device=dev)
            key = ("fourier_diff_time", spatial, L, orders)
            from neuraloperator_amd.differentiation import _build_tables
            tabs = engine.get_spectral_tables(dev, key, lambda: _build_tables(spatial, L, None,
                                                                             tuple((0, orders) for _ in range(dim))))
            rows = tuple((s, o, c, tuple(1 if v else 0 for v in od)) for s, o, c, od in terms)
            nbytes = (1 + n_out) * 8 * math.prod(kept) * groups
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            fo = lambda: engine._spectral_op(xh, tabs, rows, n_out, False, False)
            fc = lambda: dst.copy_(src)
            for _ in range(3):
                fo(), fc()
            to, tc, ro, rc = ab(fo, fc, args.reps * 5)
            lines.append(f"sc_spectral_op {method:9s} kept {'x'.join(map(str, kept)):>12s} groups {groups}: "
                         f"{to * 1e6:8.1f} us ({nbytes / to / 1e12:.2f} TB/s)  copy_ of {nbytes / 1e6:.0f} MB moved "
                         f"{tc * 1e6:8.1f} us ({nbytes / tc / 1e12:.2f} TB/s)  op / copy {to / tc:5.2f}")
            del xh, src, dst
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
