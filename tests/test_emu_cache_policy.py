"""CPU tier: the host side of the round-8 cache policies in host emulation -- which store policy and which operand
requests a contraction runs with (sc_modegemm_policy: the rule of gemm8_args), the constants the binding mirrors, and,
through the emulation's memcpy shims of the write-through / non-temporal stores and of the policy form of the LDS-DMA
request, that the policy paths of the kernels address exactly what the plain paths address (same bits, guards intact).
What the policies do to the caches exists only on the device: tests/test_gpu_cache_policy.py."""
import os
import re

import pytest
import torch

from engine_runner import emu_lib, layer_fwd_bwd
from neuraloperator_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIN = _lib.SC_GEMM_NO_SB
WT, NT, NTA, NTB = _lib.SC_GEMM_C_WT, _lib.SC_GEMM_STREAM_C, _lib.SC_GEMM_NT_A, _lib.SC_GEMM_NT_B


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


def _desc(P, Q, R, M, conj_a=0, conj_b=0):
    return dict(P=P, Q=Q, R=R, n_modes=M, a_sp=R * M, a_sr=M, a_sm=1, b_sr=Q * M, b_sq=M, b_sm=1,
                c_sp=Q * M, c_sq=M, c_sm=1, conj_a=conj_a, conj_b=conj_b)


def test_constants_mirror_the_header():
    src = open(os.path.join(ROOT, "include", "sc_engine.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    found = {}
    for name, expr in re.findall(r"\b(SC_(?:PLAN|GEMM)_[A-Z0-9_]+)\s*=\s*([0-9]+(?:\s*<<\s*[0-9]+)?)", src):
        found[name] = eval(expr)                     # digits and << only (the pattern admits nothing else)
    for name in ("SC_PLAN_PLAIN_CACHE_POLICY", "SC_GEMM_C_WT", "SC_GEMM_NT_A", "SC_GEMM_NT_B"):
        assert name in found, name
    for name, value in found.items():
        assert getattr(_lib, name) == value, name
    # the new bits collide with nothing: one bit each, outside the SC_GEMM_GRID field (bits 8..23)
    gemm = [v for k, v in found.items() if k.startswith("SC_GEMM_")]
    plan = [v for k, v in found.items() if k.startswith("SC_PLAN_")]
    for group in (gemm, plan):
        assert len(set(group)) == len(group) and all(v & (v - 1) == 0 for v in group)
    assert all(not (v & _lib.SC_GEMM_GRID(0xffff)) for v in gemm)
    assert "sc_modegemm_policy" in _lib.ScEngineLib.SYMBOLS
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in ("SC_PLAN_PLAIN_CACHE_POLICY", "SC_GEMM_C_WT", "SC_GEMM_NT_A", "SC_GEMM_NT_B", "sc_modegemm_policy"):
        assert name in text, name


def test_host_rule(lib):
    one = _desc(32, 32, 16, 8)
    assert lib.modegemm_policy(flags=PIN, **one) == 0
    assert lib.modegemm_policy(flags=PIN | WT, **one) == 2
    assert lib.modegemm_policy(flags=PIN | NT, **one) == 1
    assert lib.modegemm_policy(flags=PIN | NT | WT, **one) == 1            # nobody reads C next: non-temporal wins
    assert lib.modegemm_policy(flags=PIN | NTA, **one) == 4
    assert lib.modegemm_policy(flags=PIN | NTB, **one) == 8
    assert lib.modegemm_policy(flags=PIN | WT | NTA | NTB, **one) == 14
    # two column blocks share A, two row blocks share B
    assert lib.modegemm_policy(flags=PIN | NTA | NTB, **_desc(32, 64, 16, 8)) == 8
    assert lib.modegemm_policy(flags=PIN | NTA | NTB, **_desc(64, 32, 16, 8)) == 4
    assert lib.modegemm_policy(flags=PIN | NTA | NTB, **_desc(64, 64, 16, 8)) == 0
    assert lib.modegemm_policy(flags=PIN | NTA | NTB, **_desc(33, 32, 16, 8)) == 4      # one ragged row more: B has two readers
    # the metric shape: forward product (W = B, one row block) and the gradient of the spectrum
    M = 2112
    assert lib.modegemm_policy(flags=WT | NTB, **_desc(32, 64, 64, M)) == 2 | 8
    # the 8-wave shape (>= 8 tiles, modes a multiple of 16) keeps its one request form; the store policy holds
    wide = _desc(32, 256, 16, 16)
    assert lib.modegemm_path(flags=PIN, **wide) == 2
    assert lib.modegemm_policy(flags=PIN | WT | NTB, **wide) == 2
    # other routes: no policy
    assert lib.modegemm_policy(flags=PIN | _lib.SC_GEMM_NO_STREAM | WT, **one) == -1
    assert lib.modegemm_policy(flags=_lib.SC_GEMM_FORCE_VALU | WT, **one) == -1


def _crand(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, 2, generator=g)


@pytest.mark.parametrize("dims", [(32, 32, 4, 8), (32, 32, 5, 16), (28, 20, 7, 8), (32, 64, 6, 8), (64, 32, 6, 8)],
                         ids=lambda d: "P%d_Q%d_R%d_M%d" % d)
def test_gemm_policy_paths_same_bits(lib, dims):
    P, Q, R, M = dims
    kw = _desc(P, Q, R, M)
    a, b = _crand(P, R, M, seed=1), _crand(R, Q, M, seed=2)
    outs = []
    for flags in (PIN, PIN | WT | NTA | NTB, PIN | NT | NTA, PIN | WT | NTB):
        assert lib.modegemm_path(flags=flags, **kw) == 2
        c = torch.full((64 + P * Q * M + 64, 2), float("nan"))
        lib.modegemm(a.data_ptr(), b.data_ptr(), c[64:].data_ptr(), 0, flags=flags, **kw)
        assert torch.isnan(c[:64]).all() and torch.isnan(c[64 + P * Q * M:]).all()
        assert not torch.isnan(c[64:64 + P * Q * M]).any()
        outs.append(c)
    for o in outs[1:]:
        assert torch.equal(o[64:-64], outs[0][64:-64])


@pytest.mark.parametrize("kept", [(64, 33), (8, 5), (7, 5)], ids=lambda k: "kept%dx%d" % k)
def test_forward_transform_policy_paths_same_bits(lib, kept):
    """k_fft2d_fwd3 in emulation: 16-byte pieces, 8-byte pieces (odd block, odd start) and the sharded layout"""
    H, ni = 64, 2
    Mx, My = kept
    n = Mx * My
    torch.manual_seed(3)
    x = torch.randn(ni, H, 256)
    P = 4
    rows = -(-Mx // P)
    sh = lib.shards(P, rows, ni * rows * My)
    res = {}
    for name, flags in (("old", _lib.SC_PLAN_PLAIN_CACHE_POLICY), ("new", 0)):
        plan = lib.plan_create([H, 256], [Mx, My], flags=flags)
        assert lib.plan_kernel_name(plan, 0) == "k_fft2d_fwd3"
        for mode in (_lib.SC_FWD_SCALED, _lib.SC_FWD_ADJ_C2R):
            for shift in (0, 1):
                buf = torch.full((64 + shift + ni * n + 64, 2), float("nan"))
                lib.transform_forward(plan, mode, x.data_ptr(), buf[64 + shift:].data_ptr(), ni, 0)
                assert torch.isnan(buf[:64 + shift]).all() and torch.isnan(buf[64 + shift + ni * n:]).all()
                res[name, mode, shift] = buf[64 + shift:64 + shift + ni * n]
            sb = torch.full((64 + P * ni * rows * My + 64, 2), float("nan"))
            lib.transform_forward_sharded(plan, mode, x.data_ptr(), sb[64:].data_ptr(), ni, sh, 0)
            assert torch.isnan(sb[:64]).all() and torch.isnan(sb[64 + P * ni * rows * My:]).all()
            res[name, mode, "sharded"] = sb[64:64 + P * ni * rows * My]
        lib.plan_destroy(plan)
    for (name, mode, key), v in res.items():
        if name == "new":
            assert torch.equal(v.view(torch.int32), res["old", mode, key].view(torch.int32)), (mode, key)
            if key != "sharded":
                assert not torch.isnan(v).any()


_CHILD = """
import sys, torch
sys.path.insert(0, sys.argv[1])
from engine_runner import emu_lib, layer_fwd_bwd
lib = emu_lib()
t = torch.load(sys.argv[2])
out = layer_fwd_bwd(lib, t["x"], t["w"], t["bias"], t["g"], t["kept"], t["kept"], flags=0)
torch.save([o.contiguous() for o in out], sys.argv[3])
"""


def test_layer_sites_behind_the_measurement_switch_same_bits(lib, tmp_path):
    """The contraction sites of sc_layer_forward / _backward (yhat / gxhat store policy, non-temporal weight requests)
    are off in the product and reachable only through SC_POLICY_SITES / SC_POLICY_NT of a -DSC_DIAG build -- which the
    emulation library is.  The switch is read once per process, so a child runs the step with every site on (yhat
    non-temporal, gxhat write-through, both weight sites) at a shape whose backward pass is the fused pair launch with
    its bias job; this process runs the default.  Same bits."""
    import subprocess
    import sys
    B, C, kept = 8, 16, [8, 8]
    Mk = kept[0] * kept[1]
    d0 = dict(P=C, Q=C, R=B, n_modes=Mk, a_sp=Mk, a_sr=C * Mk, a_sm=1, conj_a=1, b_sr=C * Mk, b_sq=Mk, b_sm=1,
              c_sp=C * Mk, c_sq=Mk, c_sm=1, flags=_lib.SC_GEMM_STREAM_C)
    d1 = dict(P=B, Q=C, R=C, n_modes=Mk, a_sp=C * Mk, a_sr=Mk, a_sm=1, b_sr=Mk, b_sq=C * Mk, b_sm=1, conj_b=1,
              c_sp=C * Mk, c_sq=Mk, c_sm=1, flags=_lib.SC_GEMM_C_WT | _lib.SC_GEMM_NT_B)
    assert lib.modegemm_pair_path(d0, d1) == 1
    torch.manual_seed(5)
    t = dict(x=torch.randn(B, C, 64, 256), g=torch.randn(B, C, 64, 256), w=torch.randn(C, C, *kept, dtype=torch.cfloat),
             bias=torch.randn(C, 1, 1), kept=kept)
    torch.save(t, tmp_path / "in.pt")
    env = dict(os.environ, SC_POLICY_SITES="63", SC_POLICY_NT="4")
    subprocess.run([sys.executable, "-c", _CHILD, os.path.join(ROOT, "tests"), str(tmp_path / "in.pt"), str(tmp_path / "out.pt")],
                   env=env, check=True, timeout=600)
    got = torch.load(tmp_path / "out.pt")
    ref = layer_fwd_bwd(lib, t["x"], t["w"], t["bias"], t["g"], kept, kept, flags=0)
    for name, a, b in zip(("y", "gx", "gw", "gbias", "xhat"), got, ref):
        assert torch.equal(a, b), name


def test_layer_step_restore_bit_same_bits(lib):
    B, C, m = 4, 8, 8
    kept = [m, m // 2 + 1]
    torch.manual_seed(4)
    x, g = torch.randn(B, C, 64, 256), torch.randn(B, C, 64, 256)
    w = torch.randn(C, C, *kept, dtype=torch.cfloat)
    bias = torch.randn(C, 1, 1)
    old = layer_fwd_bwd(lib, x, w, bias, g, kept, kept, flags=_lib.SC_PLAN_PLAIN_CACHE_POLICY)
    new = layer_fwd_bwd(lib, x, w, bias, g, kept, kept, flags=0)
    for name, a, b in zip(("y", "gx", "gw", "gbias", "xhat"), new, old):
        assert torch.equal(a, b), name
