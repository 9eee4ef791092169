"""CPU tier: the attention kernel integral kernels (sc_kernels_attn.h) in host emulation through the C-ABI against the
float64 helper (tests/attention_reference.py): free-standing descriptors at the chunk and tile edges, every lane layout
and rotary form, weights, n_qry != n_src, a point of zeros, the route, every refusal before any launch, bit-identical
repeats, one gradient alone.  The emulation runs one OS thread per lane: tiny extents."""
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


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_float64_helper(emu, name):
    cfg = CASES[name]
    args = ar.desc_inputs(cfg, 41)
    got = ar.run_descriptor(emu, cfg, *args)
    assert all(bool(torch.isfinite(t).all()) for t in got)               # every element was written
    errs = ar.desc_errors(got, cfg, args)
    print(name, " ".join(f"{k} {e:.1e}" for k, e in errs.items()))
    assert max(errs.values()) <= ar.BAR, errs


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
