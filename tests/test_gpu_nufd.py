"""GPU tier: the point-cloud finite differences on an MI355X.  The descriptor lists of tests/test_emu_nufd.py at the same
bars (tests/nufd_cases.py, tests/nufd_reference.py), every recorded fixture through NonUniformFD and non_uniform_fd on
the engine route, bit-identical repeats, one step replayed from a captured graph, and a 20 000-point build whose peak
allocation shows that nothing N x N is formed."""
import numpy as np
import pytest
import torch

import nufd_cases as nc
import nufd_reference as nr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("name", sorted(nr.KNN_CASES))
def test_knn(name):
    nc.run_knn(name, DEV)


@pytest.mark.parametrize("name", sorted(nr.STENCIL_CASES))
def test_stencil(name):
    nc.run_stencil(name, DEV)


def test_lattice_of_exact_ties():
    nc.run_lattice(DEV)


def test_collinear_cloud_is_flagged():
    from neuraloperator_amd import differentiation as D
    nc.run_line(DEV)
    fd = D.NonUniformFD(torch.from_numpy(nr.line_points(40)).to(DEV), derivative_indices=[0, 1])
    assert fd.on_engine() and fd.ill_posed().tolist() == list(range(40))


@pytest.mark.parametrize("name", sorted(nr.CASES))
def test_fixtures_on_the_engine_route(name):
    from neuraloperator_amd import differentiation as D
    cfg = nr.CASES[name]
    kw = dict(num_neighbors=cfg["k"], derivative_indices=cfg["deriv"], radius=cfg["radius"], regularize_lstsq=cfg["reg"])
    ref, (points, values, g) = nr.fixture_results(name)
    p = torch.from_numpy(points).to(DEV)
    v = torch.from_numpy(values[0]).to(DEV).requires_grad_()
    with D.route("engine"):
        fd = D.NonUniformFD(p, **kw)
        der = fd(v)
        der.backward(torch.from_numpy(g[:, 0]).to(DEV))
        assert not set(fd.ill_posed().tolist()) - set(np.nonzero(ref["excluded"])[0].tolist())
        nr.check(name, ref, values, cfg["k"], _np(fd.indices), _np(fd._stencil.d2), _np(fd.fd_weights),
                 _np(der)[:, None], _np(v.grad)[None])
        idx, w = D.get_non_uniform_fd_weights(p, **kw)                      # the functions: the same bits, built again
        assert torch.equal(idx, fd.indices) and torch.equal(w, fd.fd_weights)
        assert torch.equal(D.non_uniform_fd(p, v.detach(), **kw), der.detach())
        assert torch.equal(fd(v.detach()), der.detach())


def test_a_step_replays_from_a_captured_graph():
    """apply + backward hold no host read and no allocation the capture cannot take: the replay equals the eager step"""
    from neuraloperator_amd import differentiation as D
    cfg = nr.CASES["n257_d3_k12"]
    points, values, g = nr.case_inputs(cfg)
    fd = D.NonUniformFD(torch.from_numpy(points).to(DEV), cfg["k"], cfg["deriv"])
    batch = np.stack([values, 0.5 * values, -values])
    v = torch.from_numpy(batch).to(DEV).requires_grad_()
    cot = torch.from_numpy(np.stack([g, g, 2 * g], 1)).to(DEV)

    def step():
        v.grad = None
        out = fd(v)
        out.backward(cot)
        return out.detach(), v.grad

    eager = [t.clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                               # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grad = step()
    for _ in range(2):
        out.zero_()
        grad.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager[0]) and torch.equal(grad, eager[1])


def test_gino_sized_build_allocates_nothing_quadratic():
    """N = 20 000, d = 3, k = 16: an N x N fp32 tensor would be 1.6 GB.  The stencil keeps indices (8 N k bytes), d2 (4),
    weights (4 per derivative, 3 here: 12), the transpose's perm (4) and, while it is built, row_of_edge (4), the flat
    splits and the transpose's workspace (4 N k + O(N)): 36 N k + O(N) bytes at the peak, below the 64 N k allowed.
    256 sampled points are compared with the helper."""
    from neuraloperator_amd import differentiation as D
    n, d, k, deriv = 20000, 3, 16, [0, 1, 2]
    points = np.random.default_rng(7).random((n, d), dtype=np.float32)
    p = torch.from_numpy(points).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fd = D.NonUniformFD(p, k, deriv)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak allocation of the build: {peak / (n * k):.1f} N k bytes ({peak / 2 ** 20:.1f} MiB)")
    assert peak <= 64 * n * k
    sample = np.random.default_rng(8).permutation(n)[:256]
    ridx, rd2 = nr.sorted_neighbours(points, points[sample], count=k + 1)
    dist = np.sqrt(rd2)
    tie = dist[:, k] - dist[:, k - 1] < nr.BAND * dist[:, k]
    P = points.astype(np.float64)
    A = np.ones((256, d + 1, k))
    A[:, 1:, :] = np.transpose(P[ridx[:, :k]] - P[sample][:, None], (0, 2, 1))
    scaled = A.copy()
    scaled[:, 1:, :] /= dist[:, k - 1, None, None]
    s = np.linalg.svd(scaled, compute_uv=False)
    inc = ~tie & (s[:, 0] <= nr.MAX_COND * s[:, -1])
    assert inc.mean() >= 0.99
    G = A @ np.transpose(A, (0, 2, 1))
    E = np.zeros((4, 3))
    E[1:] = np.eye(3)
    w = np.transpose(np.transpose(A, (0, 2, 1)) @ np.linalg.solve(G, E[None].repeat(256, 0)), (0, 2, 1))
    idx, got = _np(fd.indices)[sample], _np(fd.fd_weights)[sample]
    assert nr.order_ok(_np(fd.indices), _np(fd._stencil.d2)) and fd.ill_posed().numel() == 0
    assert nr.same_sets(idx[inc], ridx[inc, :k]).all()
    e_w = nr.rel_l2(nr.match_by_index(idx[inc], got[inc], ridx[inc, :k]), w[inc])
    print(f"weights of 256 sampled points: {e_w:.2e}")
    assert e_w <= 1e-5
