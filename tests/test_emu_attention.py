"""CPU tier: the attention kernel integral kernels (sc_kernels_attn.h) in host emulation through the C-ABI against the
float64 helper (tests/attention_reference.py): free-standing descriptors at the chunk and tile edges, every lane layout
and rotary form, weights, n_qry != n_src, a point of zeros, the route, every refusal before any launch, bit-identical
repeats, one gradient alone; and the part of the kernel table (ar.ATTN_KERNEL_CASES, emu=True) the thread-per-lane
emulation can afford, on guarded buffers at the row and element bounds of DESIGN 3.26, with the workspace's
intermediates.  The emulation runs one OS thread per lane: tiny extents."""
import ctypes

import pytest
import torch

import attention_reference as ar
from emu_engine import engine_on_emulation
from neuraloperator_amd import _lib

CASES = ar.DESC_CASES


@pytest.fixture(scope="module")
def emu():
    with engine_on_emulation() as lib:
        yield lib


def test_the_case_table_names_the_edges():
    ns = {c["n_src"] for c in CASES.values()}
    assert {1, ar.TILE + 1, ar.CHUNK - 1, ar.CHUNK, ar.CHUNK + 1, 2 * ar.CHUNK + 1} <= ns
    assert ar.chunks(ar.CHUNK) == 1 and ar.chunks(ar.CHUNK + 1) == 2 and ar.chunks(2 * ar.CHUNK + 1) == 3
    assert {2, 4, 12, 32} <= {c["d"] for c in CASES.values()}
    assert {0, 1, 2} == {c["rotary"] for c in CASES.values()}
    assert any((c["heads"] * c["d"]) % 64 for c in CASES.values()) and any(c["batch"] == 3 for c in CASES.values())
    assert any(c["n_qry"] != c["n_src"] for c in CASES.values())
    assert any(ar.route_of(c["d"]) == ar.MFMA and c["n_src"] % ar.KSTEP for c in CASES.values())
    # the kernel table (the device runs all of it, the emulation the cases with emu=True)
    K = ar.ATTN_KERNEL_CASES.values()
    on = lambda route, same=True: {c["n_src"] for c in K if ar.route_of(c["d"]) == route and                # noqa: E731
                                   (c["n_src"] == c["n_qry"]) == same}
    for d in (12, 32, 64, 128):                                          # T - 1, T, T + 1, 2 T, 2 T + 1 for T = 32, 128, 64
        T = ar.tile_of(d)
        assert T == {12: 32, 32: 128, 64: 128, 128: 64}[d]
        assert {T - 1, T, T + 1, 2 * T, 2 * T + 1} <= {c["n_src"] for c in K if c["d"] == d}, d
    for route in (ar.VECTOR, ar.MFMA):
        assert {255, 256, 257, 256 + 31, 256 + 33, 511, 512, 513, 8 * 256 + 1} <= on(route), route
        assert ar.chunks(8 * ar.CHUNK + 1) == 9
        pairs = {(c["n_src"], c["n_qry"]) for c in K if ar.route_of(c["d"]) == route}
        assert {(600, 40), (40, 600)} <= pairs and ar.chunks(600) == 3 and ar.chunks(40) == 1
        assert {1, 2, 3} <= on(route)
    assert {(600, 40), (40, 600)} <= {(c["n_src"], c["n_qry"]) for c in K if c["d"] == 128}
    assert {2, 4, 28, 30, 34, 36, 60, 62, 66, 68, 100, 124, 126, 32, 64, 128} <= {c["d"] for c in K}
    for d in ar.VECTOR_D + ar.MFMA_D:
        assert {c["rotary"] for c in K if c["d"] == d} >= ({0, 1, 2} if d % 4 == 0 else {0, 1}), d
    for d in (100, 124, 128):                                            # h > 0, a second batch and weights on DP = 128
        assert any(c["d"] == d and c["heads"] == 3 and c["batch"] == 2 and c["weights"] for c in K), d
    assert any((c["heads"] * c["d"]) % 32 for c in K) and any(c["weights"] == "signed" for c in K)
    assert any(c["zero_point"] is not None and c["d"] == 64 for c in K) and any(c["const_row"] is not None for c in K)
    for d in (12, 32, 128):
        T = ar.tile_of(d)
        assert {0, T - 1, T, 2 * T} <= {c["mark_g"] for c in K if c["d"] == d} and any(c["mark_q"] == T for c in K if c["d"] == d)
    assert sorted(ar.dp_of(ar.ATTN_KERNEL_CASES[n]["d"]) for n in ar.WANT_CASES.values()) == [32, 32, 64, 64, 128, 128]
    assert all(ar.ATTN_KERNEL_CASES[n]["n_src"] == ar.tile_of(ar.ATTN_KERNEL_CASES[n]["d"]) + 1 for n in ar.WANT_CASES.values())
    assert len(ar.WANT_SUBSETS) == 7 and (True, True, True) in ar.WANT_SUBSETS
    # the emulation's share: a case per DP of each route, both cross directions at D = 12, the marked points
    E = [c for c in K if c["emu"]]
    assert {(ar.route_of(c["d"]), ar.dp_of(c["d"])) for c in E} == {(r, p) for r in (ar.VECTOR, ar.MFMA) for p in (32, 64, 128)}
    assert {(600, 40), (40, 600)} <= {(c["n_src"], c["n_qry"]) for c in E if c["d"] == 12}
    assert sum(c["mark_g"] is not None for c in E) >= 8 and sum(c["mark_q"] is not None for c in E) >= 2


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_float64_helper(emu, name):
    cfg = CASES[name]
    args = ar.desc_inputs(cfg, 41)
    got = ar.run_descriptor(emu, cfg, *args)
    assert all(bool(torch.isfinite(t).all()) for t in got)               # every element was written
    errs = ar.desc_errors(got, cfg, args)
    print(name, " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    assert max(errs.values()) <= ar.BAR, errs


EMU_KERNEL_CASES = sorted(n for n, c in ar.ATTN_KERNEL_CASES.items() if c["emu"])


@pytest.mark.parametrize("name", EMU_KERNEL_CASES)
def test_kernel_table_on_guarded_buffers_at_the_row_and_element_bounds(emu, name):
    got, stats = ar.run_kernel_case(emu, name)
    assert set(stats) == set(ar.TENSORS)


@pytest.mark.parametrize("kernel", sorted(ar.WANT_CASES))
def test_every_subset_of_the_gradients_gives_the_bits_of_all_three(emu, kernel):
    """the seven non-empty subsets of (gq, gk, gv) at n = T + 1: the wanted ones bit for bit those of the all-three run,
    the others' guarded buffers and the workspace regions nobody needs untouched (asserted by the guarded run)"""
    name = ar.WANT_CASES[kernel]
    full, _ = ar.run_kernel_case(emu, name)
    for want in ar.WANT_SUBSETS[:-1]:
        part, _ = ar.run_kernel_case(emu, name, want=want)
        for key, w in zip(("gq", "gk", "gv"), want):
            assert (part[key] is not None) == w and (not w or torch.equal(part[key], full[key])), (want, key)
        assert all(part[key] is None or torch.equal(part[key], full[key]) for key in ("u", "dots", "dots_t", "g_dots", "g_dots_t"))


def test_a_point_of_zeros_adds_exactly_nothing_on_the_matrix_cores(emu):
    """the zero-point property at D = 64: dots bit for bit the dots of the cloud without the point (one chunk each)"""
    name = "zero_point_d64_one_chunk"
    cfg = ar.ATTN_KERNEL_CASES[name]
    (q, k, v, ps, pq, f, sc, w, g), _ = ar.kernel_reference(name)
    z = cfg["zero_point"]
    assert ar.route_of(cfg["d"]) == ar.MFMA and ar.chunks(cfg["n_src"]) == 1
    assert float(k[:, z].abs().max()) == 0.0 == float(v[:, z].abs().max())
    full = ar.run_descriptor(emu, cfg, q, k, v, ps, pq, f, sc, w, g, guard=True)
    keep = [i for i in range(cfg["n_src"]) if i != z]
    less = dict(cfg, n_src=cfg["n_src"] - 1, zero_point=None)
    part = ar.run_descriptor(emu, less, q, k[:, keep], v[:, keep], ps[:, keep], pq, f, sc, w, g, want=(False, False, True),
                             guard=True)
    assert torch.equal(full[1], part[1]) and all(bool(torch.isfinite(t).all()) for t in full[:5])


def test_a_point_of_zeros_adds_exactly_nothing(emu):
    """k = v = 0 at one point: the norm gives exactly 0 there and a product with 0 changes no sum, so dots is bit for bit
    the dots of the cloud without the point (one chunk: the other points keep their order); every gradient is finite"""
    cfg = CASES["zero_point_d4_rot2"]
    q, k, v, ps, pq, f, sc, w, g = ar.desc_inputs(cfg, 43)
    z = cfg["zero_point"]
    assert float(k[:, z].abs().max()) == 0.0 == float(v[:, z].abs().max())
    full = ar.run_descriptor(emu, cfg, q, k, v, ps, pq, f, sc, w, g)
    keep = [i for i in range(cfg["n_src"]) if i != z]
    less = dict(cfg, n_src=cfg["n_src"] - 1, zero_point=None)
    part = ar.run_descriptor(emu, less, q, k[:, keep], v[:, keep], ps[:, keep], pq, f, sc, w, g, want=(False, False, True))
    assert torch.equal(full[1], part[1])
    assert all(bool(torch.isfinite(t).all()) for t in full)


@pytest.mark.parametrize("name", ["n_one_above_a_chunk_d12_h2_rot2_weights", "cross_70_to_45_d32_h2_rot2_weights",
                                  "d36_second_lane_layout_no_rotary", "mfma_d64_odd_points_no_rotary"])
def test_repeats_are_bit_identical_and_one_gradient_alone_is_the_same(emu, name):
    cfg = CASES[name]
    args = ar.desc_inputs(cfg, 42)
    a, c = ar.run_descriptor(emu, cfg, *args), ar.run_descriptor(emu, cfg, *args)
    assert all(torch.equal(u, v) for u, v in zip(a, c))
    for i in range(3):                                                   # gq / gk / gv alone, then all but it
        want = tuple(j == i for j in range(3))
        one = ar.run_descriptor(emu, cfg, *args, want=want)
        assert torch.equal(one[2 + i], a[2 + i]) and sum(t is not None for t in one[2:]) == 1
        two = ar.run_descriptor(emu, cfg, *args, want=tuple(not w for w in want))
        assert two[2 + i] is None and all(torch.equal(two[2 + j], a[2 + j]) for j in range(3) if j != i)


def test_route_of_a_descriptor(emu):
    D = _lib.ScEngineLib.attn_desc
    base = dict(batch=2, n_src=100, n_qry=50, heads=3)
    for d in range(2, 129, 2):
        for rotary in (0, 1, 2):
            want = 0 if rotary == 2 and d % 4 else ar.route_of(d)
            assert emu.attn_path(D(head_dim=d, rotary=rotary, **base)) == want, (d, rotary)
    assert ar.VECTOR == _lib.SC_ATTN_PATH_VECTOR and ar.MFMA == _lib.SC_ATTN_PATH_MFMA
    assert [d for d in range(2, 129, 2) if ar.route_of(d) == ar.MFMA] == [32, 64, 128]


def test_refusals_before_any_launch(emu):
    L, D = emu.lib, _lib.ScEngineLib.attn_desc
    buf = torch.zeros(1 << 16)
    p, n = buf.data_ptr(), buf.numel() * 4
    good = dict(batch=2, n_src=9, n_qry=7, heads=2, head_dim=4, rotary=2, has_weights=1)
    sc = ctypes.c_float(64.0)
    bad = [dict(head_dim=3), dict(head_dim=0), dict(head_dim=1), dict(head_dim=130), dict(head_dim=-2),
           dict(head_dim=6), dict(head_dim=2),                                    # rotary = 2 needs head_dim % 4 == 0
           dict(rotary=3), dict(rotary=-1), dict(has_weights=2), dict(batch=0), dict(heads=0), dict(n_src=0),
           dict(n_qry=0), dict(n_src=1 << 31), dict(n_qry=1 << 31),              # beyond 32-bit indices
           dict(n_src=1 << 29), dict(n_qry=1 << 29), dict(batch=1 << 28), dict(batch=40000), dict(heads=40000)]
    for change in bad:
        d = D(**{**good, **change})
        assert L.sc_attn_path(ctypes.byref(d)) == 0, change
        assert L.sc_attn_workspace_bytes(ctypes.byref(d)) == 0, change
        assert L.sc_attn_forward(ctypes.byref(d), p, p, p, p, p, p, sc, p, p, p, p, n, None) != 0, change
        assert "sc_engine" in L.sc_last_error().decode()
        assert L.sc_attn_backward(ctypes.byref(d), p, p, p, p, p, p, sc, p, p, p, p, p, p, p, n, None) != 0, change
    ok = ctypes.byref(D(**good))
    assert L.sc_attn_path(None) == 0 and L.sc_attn_workspace_bytes(None) == 0
    assert L.sc_attn_forward(None, p, p, p, p, p, p, sc, p, p, p, p, n, None) != 0
    need = L.sc_attn_workspace_bytes(ok)
    assert need == 4 * 2 * 2 * 16 * (1 + 3)
    #             q  k  v  ps pq f  w  u  dots ws
    for i in range(10):                                                  # every pointer is required by this descriptor
        args = [p] * 10
        args[i] = None
        assert L.sc_attn_forward(ok, *args[:6], sc, *args[6:], n, None) != 0, i
    assert L.sc_attn_forward(ok, p, p, p, p, p, p, sc, p, p, p, p, 63, None) != 0             # workspace too small
    #             q  k  v  ps pq f  w  dots gu gq gk gv ws
    full = [p] * 13
    for i in (3, 4, 5, 6, 8, 12):                                        # positions, inv_freq, weights, gu, workspace
        args = list(full)
        args[i] = None
        assert L.sc_attn_backward(ok, *args[:6], sc, *args[6:], n, None) != 0, i
    for i in (0, 1, 2):                                                  # q, k, v: needed for gk / gv
        args = list(full)
        args[i] = None
        assert L.sc_attn_backward(ok, *args[:6], sc, *args[6:], n, None) != 0, i
    args = list(full)
    args[7] = None                                                       # dots: needed for gq
    assert L.sc_attn_backward(ok, *args[:6], sc, *args[6:], n, None) != 0
    args = list(full)
    args[9] = args[10] = args[11] = None                                 # no gradient is wanted
    assert L.sc_attn_backward(ok, *args[:6], sc, *args[6:], n, None) != 0
    assert L.sc_attn_backward(ok, *full[:6], sc, *full[6:], need - 1, None) != 0
    # a descriptor without rotary and weights needs neither positions, inv_freq nor weights
    plain = ctypes.byref(D(**{**good, "rotary": 0, "has_weights": 0}))
    assert float(buf.abs().sum()) == 0.0                                 # no refused call wrote anything
    assert L.sc_attn_forward(plain, p, p, p, None, None, None, sc, None, p, p, p, n, None) == 0
