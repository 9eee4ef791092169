"""The graph neural operator layer on one MI355X, for manual use (no test runs this):

    python scripts/gno_time.py [--iters 50] [--out profiles/gno.txt] [--search-only]

Per shape: the engine's radius search, first layer by point (sc_edge_lift) and fused reduce (sc_csr_reduce), each beside
a device-to-device copy of its own algorithmic bytes, and a whole GNOBlock forward + backward beside the reference's
formula written as a torch chain on the same GPU (dense cdist search, indexing, the MLP over edges, index_add_ in place of
the Python loop of segment_csr).  Shapes: 3586 surface points against 32^3 and 64^3 grid queries at radius 0.033 (the
GINO in direction) and the reverse (the out direction).  Then the search alone on both routes (method="brute" and
method="grid", the same bytes out): those four shapes, a synthetic 100 000-point surface against 64^3 in both directions,
and a sweep over the number of data points at 64^3 queries that shows where the routes cross (engine.radius_route's
threshold is set from it).  --search-only skips the first part.  --mlp adds (and --mlp-only runs alone) the kernel
MLP's two routes: a GNOBlock forward + backward on kernel_route "edges" and "fused" with the peak of
torch.cuda.max_memory_allocated of each, at those six shapes for the widths [80, 80, 80] and [512, 256], and the fused
route's chunk size at the 3.76 M-edge shape for workspaces of 16 / 32 / 64 / 128 MiB (engine.edge_mlp_route and the
default chunk are set from this table).  Events around the whole loop after a warm-up."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuraloperator_amd import GNOBlock, engine  # noqa: E402
from neuraloperator_amd.gno import kernel_route  # noqa: E402

N_SURF, RADIUS, CH = 3586, 0.033, 32


def timed(fn, iters, warmup=5):
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


def chain_search(data, queries, radius):
    d = torch.cdist(queries, data)
    hit = d <= radius
    return {"neighbors_index": hit.nonzero()[:, 1], "neighbors_row_splits": F.pad(hit.sum(1).cumsum(0), (1, 0))}


def chain_block(block, y, x, f, chunk=8192):
    """the reference's formula, dense search in query chunks so that 64^3 x 3586 distances fit"""
    idx, rows = [], []
    for q0 in range(0, x.shape[0], chunk):
        hit = (torch.cdist(x[q0:q0 + chunk], y) <= block.radius).nonzero()
        rows.append(hit[:, 0] + q0)
        idx.append(hit[:, 1])
    idx, rows = torch.cat(idx), torch.cat(rows)
    ye, xe = block.pos_embedding(y), block.pos_embedding(x)
    k = block.integral_transform.channel_mlp(torch.cat([ye[idx], xe[rows]], -1)) * f[:, idx]
    return torch.zeros(f.shape[0], x.shape[0], k.shape[-1], device=k.device).index_add_(1, rows, k)


def sphere_surface(n, gen):
    """n points on the sphere of radius 0.3 around the centre of the unit box: a closed surface mesh's worth of points"""
    v = torch.randn(n, 3, generator=gen)
    return (0.5 + 0.3 * v / v.norm(dim=1, keepdim=True)).float().contiguous()


def lattice_grid(res, dev):
    ax = torch.linspace(0, 1, res)
    return torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).to(dev)


def search_routes(lines, tag, y, x, iters):
    """one row: the search alone on both routes, after checking that they return the same bytes"""
    a = engine.radius_search(y, x, RADIUS, True, method="brute")
    b = engine.radius_search(y, x, RADIUS, True, method="grid")
    assert all(torch.equal(a[k], b[k]) for k in a), tag
    n, m = y.shape[0], x.shape[0]
    it = max(3, min(iters, int(2e11 / (n * m))))            # the brute-force route at 2.6e10 pair tests takes a while
    t_b = timed(lambda: engine.radius_search(y, x, RADIUS, True, method="brute"), it, warmup=2)
    t_g = timed(lambda: engine.radius_search(y, x, RADIUS, True, method="grid"), it, warmup=2)
    lines.append(f"{tag:>22s} {n:8d} {m:8d} {n * m:10.3g} {a['neighbors_index'].numel():9d} {t_b:10.1f} {t_g:10.1f} "
                 f"{t_b / t_g:7.2f}  {engine.radius_route(n, m, 3)}")
    print(lines[-1], flush=True)


def search_table(dev, iters):
    g = torch.Generator().manual_seed(0)
    surf = (0.25 + 0.5 * torch.rand(N_SURF, 3, generator=g)).to(dev)
    lines = ["", "search alone, both routes (weights included; the host's 8-byte read of the edge count is inside)",
             f"{'shape':>22s} {'n':>8s} {'m':>8s} {'n*m':>10s} {'edges':>9s} {'brute us':>10s} {'grid us':>10s} "
             f"{'b/g':>7s}  auto"]
    for res in (32, 64):
        grid = lattice_grid(res, dev)
        search_routes(lines, f"in {N_SURF}->{res}^3", surf, grid, iters)
        search_routes(lines, f"out {res}^3->{N_SURF}", grid, surf, iters)
    big, grid = sphere_surface(100_000, g).to(dev), lattice_grid(64, dev)
    search_routes(lines, "in 100000->64^3", big, grid, iters)
    search_routes(lines, "out 64^3->100000", grid, big, iters)
    lines += ["", "crossover sweep: n surface points against m grid queries"]
    for res in (32, 64):
        grid = lattice_grid(res, dev)
        for n in (256, 512, 1024, 2048, 4096, 8192, 16384, 32768):
            search_routes(lines, f"sweep {n}->{res}^3", sphere_surface(n, g).to(dev), grid, iters)
    return lines


MLP_WIDTHS = ([80, 80, 80], [512, 256])


def block_step(block, y, x, f, nbrs, route):
    """forward + backward of the block's transform on precomputed neighbours (the search is the same on both routes)"""
    f.grad = None
    block.zero_grad(set_to_none=True)
    ye, xe = block.pos_embedding(y), block.pos_embedding(x)
    with kernel_route(route):
        block.integral_transform(y=ye, x=xe, neighbors=nbrs, f_y=f).sum().backward()


def mlp_routes(lines, tag, y, x, widths, iters):
    """one row: both routes of the kernel MLP, time and peak memory of a step, and what "auto" takes"""
    dev = y.device
    nbrs = engine.radius_search(y, x, RADIUS)
    E = nbrs["neighbors_index"].numel()
    block = GNOBlock(CH, CH, 3, RADIUS, channel_mlp_layers=list(widths)).to(dev)
    f = torch.randn(1, y.shape[0], CH, device=dev, requires_grad=True)
    it = max(3, min(iters, int(3e7 / max(E, 1))))
    out = {}
    for route in ("edges", "fused"):
        block_step(block, y, x, f, nbrs, route)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        t = timed(lambda: block_step(block, y, x, f, nbrs, route), it, warmup=1)
        out[route] = (t, torch.cuda.max_memory_allocated(dev) / 2 ** 20)
    work = E * sum(list(widths) + [CH])
    lines.append(f"{tag:>22s} {str(list(widths)):>14s} {E:9d} {work:10.3g} {out['edges'][0]:10.1f} {out['fused'][0]:10.1f} "
                 f"{out['edges'][0] / out['fused'][0]:7.2f} {out['edges'][1]:10.1f} {out['fused'][1]:10.1f}  "
                 f"{engine.edge_mlp_route(E, 1, list(widths) + [CH])}")
    print(lines[-1], flush=True)


def mlp_table(dev, iters):
    g = torch.Generator().manual_seed(0)
    surf = (0.25 + 0.5 * torch.rand(N_SURF, 3, generator=g)).to(dev)
    lines = ["", "kernel MLP, both routes: the transform's forward + backward on precomputed neighbours, b = 1, 32 channels",
             f"{'shape':>22s} {'widths':>14s} {'edges':>9s} {'E sum c':>10s} {'edges us':>10s} {'fused us':>10s} "
             f"{'e/f':>7s} {'edges MiB':>10s} {'fused MiB':>10s}  auto"]
    shapes = []
    for res in (32, 64):
        grid = lattice_grid(res, dev)
        shapes += [(f"in {N_SURF}->{res}^3", surf, grid), (f"out {res}^3->{N_SURF}", grid, surf)]
    big, grid = sphere_surface(100_000, g).to(dev), lattice_grid(64, dev)
    shapes += [("in 100000->64^3", big, grid), ("out 64^3->100000", grid, big)]
    for widths in MLP_WIDTHS:
        for tag, y, x in shapes:
            mlp_routes(lines, tag, y, x, widths, iters)
    lines += ["", "fused route, chunk size at in 100000->64^3 (workspace of the hidden layers; 0 = the default)",
              f"{'widths':>14s} {'workspace MiB':>14s} {'chunk_edges':>12s} {'fused us':>10s} {'peak MiB':>10s}"]
    nbrs = engine.radius_search(big, grid, RADIUS)
    for widths in MLP_WIDTHS:
        block = GNOBlock(CH, CH, 3, RADIUS, channel_mlp_layers=list(widths)).to(dev)
        f = torch.randn(1, big.shape[0], CH, device=dev, requires_grad=True)
        for mib in (0, 16, 32, 64, 128):
            engine.EDGE_MLP_CHUNK_EDGES = (mib << 20) // (8 * sum(widths)) // 128 * 128
            block_step(block, big, grid, f, nbrs, "fused")
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            t = timed(lambda: block_step(block, big, grid, f, nbrs, "fused"), 3, warmup=1)
            lines.append(f"{str(list(widths)):>14s} {mib:14d} {engine.EDGE_MLP_CHUNK_EDGES:12d} {t:10.1f} "
                         f"{torch.cuda.max_memory_allocated(dev) / 2 ** 20:10.1f}")
            print(lines[-1], flush=True)
        engine.EDGE_MLP_CHUNK_EDGES = 0
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--search-only", action="store_true")
    ap.add_argument("--mlp", action="store_true")
    ap.add_argument("--mlp-only", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    surf = (0.25 + 0.5 * torch.rand(N_SURF, 3, generator=g)).to(dev)
    lines = [f"{'shape':>22s} {'step':>14s} {'engine us':>10s} {'copy us':>9s} {'torch chain us':>15s}"]
    for res in (() if args.search_only or args.mlp_only else (32, 64)):
        ax = torch.linspace(0, 1, res)
        grid = torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3).to(dev)
        for tag, y, x in ((f"in {N_SURF}->{res}^3", surf, grid), (f"out {res}^3->{N_SURF}", grid, surf)):
            n, m = y.shape[0], x.shape[0]
            nb = engine.radius_search(y, x, RADIUS)
            E = nb["neighbors_index"].numel()
            graph = engine.CsrGraph(nb["neighbors_row_splits"], nb["neighbors_index"], n)
            rows = [("search", timed(lambda: engine.radius_search(y, x, RADIUS), args.iters),
                     copy_us(12 * (n + m) + 8 * (m + 1) + 8 * E, args.iters),
                     timed(lambda: chain_search(y, x, RADIUS), args.iters) if m * n < 2 ** 28 else float("nan"))]
            h = 128
            Py, Px, b = torch.randn(n, h, device=dev), torch.randn(m, h, device=dev), torch.randn(h, device=dev)
            rows.append(("lift h=128", timed(lambda: engine.EdgeLiftFn.apply(Py, Px, b, graph, True), args.iters),
                         copy_us(4 * h * (n + m + E) + 8 * E, args.iters), float("nan")))
            K, Fv = torch.randn(E, CH, device=dev), torch.randn(1, n, CH, device=dev)
            rows.append(("reduce c=32", timed(lambda: engine._csr_reduce(graph, K, Fv), args.iters),
                         copy_us(4 * CH * (E + n + m) + 8 * E, args.iters), float("nan")))
            block = GNOBlock(CH, CH, 3, RADIUS, channel_mlp_layers=[128, 256, 128]).to(dev)
            f = torch.randn(1, n, CH, device=dev, requires_grad=True)

            def step(fn):
                f.grad = None
                block.zero_grad(set_to_none=True)
                fn().sum().backward()
            rows.append(("block fwd+bwd", timed(lambda: step(lambda: block(y, x, f)), args.iters), float("nan"),
                         timed(lambda: step(lambda: chain_block(block, y, x, f)), max(args.iters // 5, 2))))
            for name, t_eng, t_copy, t_ref in rows:
                lines.append(f"{tag:>22s} {name:>14s} {t_eng:10.1f} {t_copy:9.1f} {t_ref:15.1f}")
                print(lines[-1], flush=True)
            lines.append(f"{tag:>22s} {'edges':>14s} {E:10d}")
    if not args.mlp_only:
        lines += search_table(dev, args.iters)
    if args.mlp or args.mlp_only:
        lines += mlp_table(dev, args.iters)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
