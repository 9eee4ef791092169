"""GPU tier: the attention kernels (sc_kernels_attn.h) at their tile, chunk and lane edges on an MI355X.  Every entry of
ar.ATTN_KERNEL_CASES runs through the C-ABI on guarded buffers (a full tile of rows of a NaN sentinel in front of and
behind u, dots, every gradient and both workspaces, compared bit for bit), the workspace's dots^T, g_dots and g_dots^T
are read back, and every tensor is held row by row at the project's bar and, without rotary, element by element at
gamma_N A with N counted in the kernel source.  Then: every subset of the gradients on each backward kernel
instantiation, bit-identical repeats, a zero point on the matrix cores, and forward + backward replayed from one captured
graph.  The last test prints the worst |err| / bound per kernel and route."""
import pytest
import torch

import attention_reference as ar

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WORST = {}                     # (route, tensor) -> (worst element ratio, case, worst row ratio, case)
# The tables are read while pytest collects.  Beside a helper without them this module still has to collect -- an error
# here would stop the collection of every other module of the suite -- and test_the_helper_holds_the_kernel_table fails.
CASES = getattr(ar, "ATTN_KERNEL_CASES", {})
WANT = getattr(ar, "WANT_CASES", {})


def test_the_helper_holds_the_kernel_table():
    assert len(CASES) >= 126 and len(WANT) == 6 and set(WANT.values()) <= set(CASES)
    assert CASES is ar.ATTN_KERNEL_CASES and WANT is ar.WANT_CASES


def _lib():
    from neuraloperator_amd import _lib as L
    return L.get_lib()


def _note(name, stats):
    cfg = ar.ATTN_KERNEL_CASES[name]
    route = "matrix-core" if ar.route_of(cfg["d"]) == ar.MFMA else "vector"
    for key, (_, row, el) in stats.items():
        e, en, r, rn = WORST.get((route, key), (0.0, "", 0.0, ""))
        if el is not None and el > e:
            e, en = el, name
        if cfg["rotary"] and row > r:
            r, rn = row, name
        WORST[(route, key)] = (e, en, r, rn)


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_table_on_guarded_buffers_at_the_row_and_element_bounds(name):
    cfg = ar.ATTN_KERNEL_CASES[name]
    lib, d = _lib(), ar.desc_of(cfg)
    assert lib.attn_path(d) == ar.route_of(cfg["d"]) == (ar.MFMA if cfg["d"] in (32, 64, 128) else ar.VECTOR)
    cmax = max(ar.chunks(cfg["n_src"]), ar.chunks(cfg["n_qry"]))
    assert lib.attn_workspace_bytes(d) == 4 * cfg["batch"] * cfg["heads"] * cfg["d"] ** 2 * (cmax + 3)
    got, stats = ar.run_kernel_case(lib, name, DEV)
    assert set(stats) == set(ar.TENSORS)
    _note(name, stats)


@pytest.mark.parametrize("kernel", sorted(WANT))
def test_every_subset_of_the_gradients_gives_the_bits_of_all_three(kernel):
    """the seven non-empty subsets of (gq, gk, gv) at n = T + 1 on each instantiation of the backward kernel: the wanted
    gradients bit for bit those of the all-three run; the guarded run asserts that the buffers of the others, dots^T
    without gq, and g_dots / g_dots^T without gk or gv keep their sentinel"""
    name, lib = ar.WANT_CASES[kernel], _lib()
    full, _ = ar.run_kernel_case(lib, name, DEV)
    for want in ar.WANT_SUBSETS[:-1]:
        part, _ = ar.run_kernel_case(lib, name, DEV, want=want)
        for key, w in zip(("gq", "gk", "gv"), want):
            assert (part[key] is not None) == w and (not w or torch.equal(part[key], full[key])), (want, key)
        assert all(part[key] is None or torch.equal(part[key], full[key]) for key in ("u", "dots", "dots_t", "g_dots", "g_dots_t"))


@pytest.mark.parametrize("name", ["lanes_d100_h3_b2_weights_no_rotary", "tile_d32_n129", "chunk_d32_n2049", "chunk_d4_n2049"])
def test_repeats_are_bit_identical(name):
    """the widest vector layout, the four-wave combine of D = 32 on the matrix cores, and nine partials on both routes"""
    cfg = ar.ATTN_KERNEL_CASES[name]
    assert name != "tile_d32_n129" or (cfg["d"] == 32 and ar.route_of(32) == ar.MFMA)
    assert "2049" not in name or ar.chunks(cfg["n_src"]) == 9
    lib = _lib()
    a, _ = ar.run_kernel_case(lib, name, DEV)
    b, _ = ar.run_kernel_case(lib, name, DEV)
    assert all(torch.equal(a[key], b[key]) for key in ar.TENSORS)


def test_a_point_of_zeros_adds_exactly_nothing_on_the_matrix_cores():
    name = "zero_point_d64_one_chunk"
    cfg, lib = ar.ATTN_KERNEL_CASES[name], _lib()
    (q, k, v, ps, pq, f, sc, w, g), _ = ar.kernel_reference(name)
    z = cfg["zero_point"]
    assert ar.route_of(cfg["d"]) == ar.MFMA and ar.chunks(cfg["n_src"]) == 1
    full = ar.run_descriptor(lib, cfg, q, k, v, ps, pq, f, sc, w, g, device=DEV, guard=True)
    keep = [i for i in range(cfg["n_src"]) if i != z]
    less = dict(cfg, n_src=cfg["n_src"] - 1, zero_point=None)
    part = ar.run_descriptor(lib, less, q, k[:, keep], v[:, keep], ps[:, keep], pq, f, sc, w, g, want=(False, False, True),
                             device=DEV, guard=True)
    assert torch.equal(full[1], part[1]) and all(bool(torch.isfinite(t).all()) for t in full[:5])


@pytest.mark.parametrize("name", ["lanes_d124_rot2", "tile_d128_n65"])
def test_forward_and_backward_replay_from_one_captured_graph(name):
    """sc_attn_forward + sc_attn_backward recorded on a side stream into one graph (a single stream: no parallel
    branches), replayed on new inputs: bit for bit the eager calls"""
    cfg, lib = ar.ATTN_KERNEL_CASES[name], _lib()
    assert cfg["n_src"] == ar.tile_of(cfg["d"]) + 1 and cfg["d"] in (124, 128)
    d = ar.desc_of(cfg)
    static = [None if t is None or isinstance(t, float) else t.to(DEV).contiguous() for t in ar.desc_inputs(cfg, 61)]
    q, k, v, ps, pq, f, _, w, g = static
    B, H, D = cfg["batch"], cfg["heads"], cfg["d"]
    outs = [torch.empty_like(q), torch.empty(B, H, D, D, device=DEV), torch.empty_like(q), torch.empty_like(k),
            torch.empty_like(v)]
    nbytes = lib.attn_workspace_bytes(d)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    p = lambda t: 0 if t is None else t.data_ptr()                                      # noqa: E731

    def launch(st):
        lib.attn_forward(d, p(q), p(k), p(v), p(ps), p(pq), p(f), 64.0, p(w), p(outs[0]), p(outs[1]), p(ws), nbytes, st)
        lib.attn_backward(d, p(q), p(k), p(v), p(ps), p(pq), p(f), 64.0, p(w), p(outs[1]), p(g), p(outs[2]), p(outs[3]),
                          p(outs[4]), p(ws), nbytes, st)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        launch(side.cuda_stream)                             # warm-up off the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        launch(torch.cuda.current_stream().cuda_stream)
    for seed in (62, 63):
        new = ar.desc_inputs(cfg, seed)
        for dst, src in zip(static, new):
            if dst is not None:
                dst.copy_(src.to(DEV))
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        eager = ar.run_descriptor(lib, cfg, *new, device=DEV)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(outs, eager))


def test_report_the_worst_ratio_per_kernel():
    """prints, per route and tensor, the worst |err| / (gamma_N A) over the cases without rotary and the worst row ratio
    ||err_row|| / (1e-5 ||A_row||) over the rotary cases (the figures of DESIGN 3.26)"""
    for (route, key), (e, en, r, rn) in sorted(WORST.items()):
        print(f"{route:12s} {key:9s} {ar.KERNEL_OF[key]:38s} element {e:.3f} ({en})  rotary row {r:.3f} ({rn})")
