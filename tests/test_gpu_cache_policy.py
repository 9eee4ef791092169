"""GPU tier (``-m gpu``): the cache policies of round 8 change no bit.

Write-through / non-temporal stores of the spectra (k_fft2d_fwd3, k_modegemm_dma, k_modegemm_dma_bwd) and non-temporal
LDS-DMA requests for read-once operands are memory-policy choices: every output must equal, bit for bit, what the same
launch gives with plain stores and default requests.  The old policy comes from SC_PLAN_PLAIN_CACHE_POLICY (plans, layer
calls) or from the absence of SC_GEMM_C_WT / SC_GEMM_NT_A / SC_GEMM_NT_B (contractions), the new one from the default
or from those flags.  Outputs sit between NaN-filled guard bands that must stay NaN.  Every comparison is torch.equal."""
import pytest
import torch

from engine_runner import layer_fwd_bwd
from neuraloperator_amd import _lib

pytestmark = pytest.mark.gpu
GUARD = 1024           # complex elements in front of and behind every output


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("GPU tier: no GPU visible")
    return _lib.get_lib()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _guarded(n, dev, shift=0):
    """(whole buffer, view of n complex elements behind GUARD + shift) -- float32 pairs, all NaN"""
    buf = torch.full((2 * GUARD + n + shift, 2), float("nan"), device=dev)
    return buf, buf[GUARD + shift:GUARD + shift + n]


def _guards_intact(buf, n, shift=0):
    return bool(torch.isnan(buf[:GUARD + shift]).all()) and bool(torch.isnan(buf[GUARD + shift + n:]).all())


def _crand(*shape, dev, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(*shape, 2, generator=g).to(dev)


def _st():
    return torch.cuda.current_stream().cuda_stream


# ---------------------------------------------------------------------------------------------- sc_modegemm
PIN = _lib.SC_GEMM_NO_SB       # keep small extents off the small-batch kernel: this file is about the streamed route
STORES = {"plain": 0, "nt": _lib.SC_GEMM_STREAM_C, "wt": _lib.SC_GEMM_C_WT}
LOADS = {"none": 0, "ntA": _lib.SC_GEMM_NT_A, "ntB": _lib.SC_GEMM_NT_B, "both": _lib.SC_GEMM_NT_A | _lib.SC_GEMM_NT_B}


def _desc(P, Q, R, M, conj_a=0, conj_b=0):
    return dict(P=P, Q=Q, R=R, n_modes=M, a_sp=R * M, a_sr=M, a_sm=1, b_sr=Q * M, b_sq=M, b_sm=1,
                c_sp=Q * M, c_sq=M, c_sm=1, conj_a=conj_a, conj_b=conj_b)


def _run_gemm(lib, a, b, kw, flags, dev):
    P, Q, M = kw["P"], kw["Q"], kw["n_modes"]
    buf, c = _guarded(P * Q * M, dev)
    assert lib.modegemm_path(flags=flags, **kw) == 2, "the streamed route is what this test is about"
    lib.modegemm(a.data_ptr(), b.data_ptr(), c.data_ptr(), _st(), flags=flags, **kw)
    torch.cuda.synchronize()
    assert _guards_intact(buf, P * Q * M)
    assert not torch.isnan(c).any()
    return c


def _accepted_r(lib, P, Q, R, M):
    """the router refuses r loops shorter than four values (gemm8_eligible): the nearest extent it accepts"""
    while lib.modegemm_path(flags=PIN, **_desc(P, Q, R, M)) != 2:
        R += 1
        assert R <= 8
    return R


@pytest.mark.parametrize("M", [8, 16], ids=["one_mode_group", "two_mode_groups"])
@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 64])
def test_modegemm_every_policy_same_bits(lib, dev, M, R):
    """P = Q = 32 (one tile: A and B both read once).  R = 1, 2, 3 are refused by the router and run as R = 4, the
    nearest extent it accepts (one stage, partly clamped); R = 5 re-reads the clamped last piece of an odd r loop."""
    P = Q = 32
    R = _accepted_r(lib, P, Q, R, M)
    kw = _desc(P, Q, R, M)
    a, b = _crand(P, R, M, dev=dev, seed=11), _crand(R, Q, M, dev=dev, seed=12)
    ref = _run_gemm(lib, a, b, kw, PIN, dev)
    assert lib.modegemm_policy(flags=PIN, **kw) == 0
    for sname, sf in STORES.items():
        for lname, lf in LOADS.items():
            want = {"plain": 0, "nt": 1, "wt": 2}[sname] | (4 if lf & _lib.SC_GEMM_NT_A else 0) | (8 if lf & _lib.SC_GEMM_NT_B else 0)
            assert lib.modegemm_policy(flags=PIN | sf | lf, **kw) == want, (sname, lname)
            got = _run_gemm(lib, a, b, kw, PIN | sf | lf, dev)
            assert torch.equal(got, ref), (sname, lname)


@pytest.mark.parametrize("P,Q,off_bit", [(32, 64, 4), (64, 32, 8), (64, 64, 12)], ids=["A_shared", "B_shared", "both_shared"])
def test_modegemm_shared_operand_keeps_default_requests(lib, dev, P, Q, off_bit):
    """two column blocks share A, two row blocks share B: the host rule must switch the non-temporal request off there"""
    R, M = 16, 8
    kw = _desc(P, Q, R, M)
    both = _lib.SC_GEMM_NT_A | _lib.SC_GEMM_NT_B
    pol = lib.modegemm_policy(flags=PIN | both | _lib.SC_GEMM_C_WT, **kw)
    assert pol == (2 | 12) & ~off_bit
    a, b = _crand(P, R, M, dev=dev, seed=13), _crand(R, Q, M, dev=dev, seed=14)
    ref = _run_gemm(lib, a, b, kw, PIN, dev)
    assert torch.equal(_run_gemm(lib, a, b, kw, PIN | both | _lib.SC_GEMM_C_WT, dev), ref)


@pytest.mark.parametrize("ca,cb", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_modegemm_conjugations(lib, dev, ca, cb):
    P, Q, R, M = 32, 32, 12, 16
    kw = _desc(P, Q, R, M, ca, cb)
    a, b = _crand(P, R, M, dev=dev, seed=15), _crand(R, Q, M, dev=dev, seed=16)
    ref = _run_gemm(lib, a, b, kw, PIN, dev)
    for sf in (_lib.SC_GEMM_C_WT, _lib.SC_GEMM_STREAM_C):
        assert torch.equal(_run_gemm(lib, a, b, kw, PIN | sf | _lib.SC_GEMM_NT_A | _lib.SC_GEMM_NT_B, dev), ref)


def test_modegemm_other_routes_ignore_the_bits(lib, dev):
    """a call that does not take the streamed kernel reports no policy and computes what it computed"""
    kw = _desc(32, 32, 16, 8)
    flags = _lib.SC_GEMM_NO_STREAM | PIN
    assert lib.modegemm_policy(flags=flags | _lib.SC_GEMM_C_WT, **kw) == -1
    a, b = _crand(32, 16, 8, dev=dev, seed=17), _crand(16, 32, 8, dev=dev, seed=18)
    out = []
    for f in (flags, flags | _lib.SC_GEMM_C_WT | _lib.SC_GEMM_NT_A | _lib.SC_GEMM_NT_B):
        buf, c = _guarded(32 * 32 * 8, dev)
        lib.modegemm(a.data_ptr(), b.data_ptr(), c.data_ptr(), _st(), flags=f, **kw)
        torch.cuda.synchronize()
        assert _guards_intact(buf, 32 * 32 * 8)
        out.append(c)
    assert torch.equal(out[0], out[1])


def test_store_helper_beyond_two_gib(lib, dev):
    """the write-through store takes a full 64-bit address per lane: C (and the transform's xhat, whose block base sits in
    a buffer resource) 2 GiB + 64 KiB into one allocation"""
    big = torch.empty((1 << 31) + (8 << 20), dtype=torch.uint8, device=dev)
    far = big[(1 << 31) + (1 << 16):].view(torch.float32)
    far.fill_(float("nan"))
    P = Q = 32
    R, M = 8, 16
    kw = _desc(P, Q, R, M)
    a, b = _crand(P, R, M, dev=dev, seed=19), _crand(R, Q, M, dev=dev, seed=20)
    ref = _run_gemm(lib, a, b, kw, PIN, dev)
    n = P * Q * M
    c = far[2 * GUARD:2 * GUARD + 2 * n]
    assert c.data_ptr() - big.data_ptr() > (1 << 31)
    lib.modegemm(a.data_ptr(), b.data_ptr(), c.data_ptr(), _st(), flags=PIN | _lib.SC_GEMM_C_WT | _lib.SC_GEMM_NT_B, **kw)
    torch.cuda.synchronize()
    assert torch.equal(c.view(-1, 2), ref)
    assert torch.isnan(far[:2 * GUARD]).all() and torch.isnan(far[2 * GUARD + 2 * n:2 * GUARD + 2 * n + 4096]).all()
    # the transform: 3 images of 64 x 33 coefficients behind the same far pointer
    far.fill_(float("nan"))
    x = torch.randn(3, 64, 256, device=dev)
    near = torch.empty(3 * 64 * 33, 2, device=dev)
    for flags, dst in ((_lib.SC_PLAN_PLAIN_CACHE_POLICY, near), (0, far[2 * GUARD:2 * GUARD + 2 * 3 * 64 * 33])):
        plan = lib.plan_create([64, 256], [64, 33], flags=flags)
        lib.transform_forward(plan, _lib.SC_FWD_SCALED, x.data_ptr(), dst.data_ptr(), 3, 0, _st())
        torch.cuda.synchronize()
        lib.plan_destroy(plan)
    assert torch.equal(far[2 * GUARD:2 * GUARD + 2 * 3 * 64 * 33].view(-1, 2), near)
    assert torch.isnan(far[:2 * GUARD]).all()
    assert torch.isnan(far[2 * GUARD + 2 * 3 * 64 * 33:2 * GUARD + 2 * 3 * 64 * 33 + 4096]).all()


# ---------------------------------------------------------------------------------------------- sc_modegemm_pair
def _pair_descs(B, Ci, Co, M, f0, f1):
    d0 = dict(P=Ci, Q=Co, R=B, n_modes=M, a_sp=M, a_sr=Ci * M, a_sm=1, conj_a=1, b_sr=Co * M, b_sq=M, b_sm=1,
              c_sp=Co * M, c_sq=M, c_sm=1, flags=f0)
    d1 = dict(P=B, Q=Ci, R=Co, n_modes=M, a_sp=Co * M, a_sr=M, a_sm=1, b_sr=M, b_sq=Co * M, b_sm=1, conj_b=1,
              c_sp=Ci * M, c_sq=M, c_sm=1, flags=f1)
    return d0, d1


def test_pair_launch_policies_same_bits_as_two_single_launches(lib, dev):
    """sc_modegemm_pair (no bias job: the C-ABI pair has none; the launch WITH its bias job is
    test_layer_step_with_the_fused_pair_and_its_bias_job below).  The
    smallest pair gemm8_pair_args lays out in whole octets of workgroups: one tile per job and 8 mode groups of 8 modes
    (n_modes = 64), extents that fill half a 32 x 32 tile."""
    shape = None
    for B, Ci, Co in ((8, 16, 16), (16, 16, 16), (16, 32, 32), (32, 32, 32)):
        if lib.modegemm_pair_path(*_pair_descs(B, Ci, Co, 64, PIN | _lib.SC_GEMM_STREAM_C, PIN)) == 1:
            shape = (B, Ci, Co)
            break
    assert shape is not None, "no candidate takes the one-launch pair"
    B, Ci, Co = shape
    M = 64
    xh, gh, w = _crand(B, Ci, M, dev=dev, seed=21), _crand(B, Co, M, dev=dev, seed=22), _crand(Ci, Co, M, dev=dev, seed=23)
    # the two single launches, round-7 policy
    d0, d1 = _pair_descs(B, Ci, Co, M, PIN | _lib.SC_GEMM_STREAM_C, PIN)
    b0, gw0 = _guarded(Ci * Co * M, dev)
    b1, gx0 = _guarded(B * Ci * M, dev)
    assert lib.modegemm_path(**d0) == 2 and lib.modegemm_path(**d1) == 2
    lib.modegemm(xh.data_ptr(), gh.data_ptr(), gw0.data_ptr(), _st(), **d0)
    lib.modegemm(gh.data_ptr(), w.data_ptr(), gx0.data_ptr(), _st(), **d1)
    torch.cuda.synchronize()
    assert _guards_intact(b0, Ci * Co * M) and _guards_intact(b1, B * Ci * M)
    for f1 in (PIN, PIN | _lib.SC_GEMM_C_WT, PIN | _lib.SC_GEMM_C_WT | _lib.SC_GEMM_NT_B, PIN | _lib.SC_GEMM_STREAM_C | _lib.SC_GEMM_NT_B,
               PIN | _lib.SC_GEMM_NT_A | _lib.SC_GEMM_NT_B):
        p0, p1 = _pair_descs(B, Ci, Co, M, PIN | _lib.SC_GEMM_STREAM_C, f1)
        assert lib.modegemm_pair_path(p0, p1) == 1
        c0, gw1 = _guarded(Ci * Co * M, dev)
        c1, gx1 = _guarded(B * Ci * M, dev)
        lib.modegemm_pair(p0, xh.data_ptr(), gh.data_ptr(), gw1.data_ptr(), p1, gh.data_ptr(), w.data_ptr(), gx1.data_ptr(), _st())
        torch.cuda.synchronize()
        assert _guards_intact(c0, Ci * Co * M) and _guards_intact(c1, B * Ci * M)
        assert torch.equal(gw1, gw0) and torch.equal(gx1, gx0), f1


# ---------------------------------------------------------------------------------------------- forward-type transform
def _to_shards(plain, P, rows):
    """(ni, Mx, My, 2) -> (P, ni, rows, My, 2); rows past Mx travel as zeros (include/sc_engine.h, sc_spectrum_shards)"""
    ni, Mx, My, _ = plain.shape
    out = torch.zeros((P, ni, rows, My, 2), device=plain.device)
    for p in range(P):
        r0, r1 = p * rows, min((p + 1) * rows, Mx)
        if r1 > r0:
            out[p, :, :r1 - r0] = plain[:, r0:r1]
    return out


@pytest.mark.parametrize("io", ["f32", "bf16_valu"])
@pytest.mark.parametrize("kept", [(64, 33), (8, 5), (7, 5)], ids=lambda k: "kept%dx%d" % k)
@pytest.mark.parametrize("ni", [1, 3])
@pytest.mark.parametrize("H", [64, 256])
def test_forward_transform_store_policy_same_bits(lib, dev, H, ni, kept, io):
    """k_fft2d_fwd3, both modes, plain and sharded layout; kept 7 x 5 (an odd number of coefficients per image) and a
    spectrum that starts 8 bytes off a 16-byte boundary take the 8-byte write-through stores"""
    Mx, My = kept
    n = Mx * My
    base = (_lib.SC_PLAN_IO_BF16 | _lib.SC_PLAN_NO_MX_FFT) if io != "f32" else 0
    x = torch.randn(ni, H, 256, device=dev)
    if io != "f32":
        x = x.bfloat16()
    P = 4
    rows = -(-Mx // P)
    sh = lib.shards(P, rows, ni * rows * My)
    res = {}
    for name, flags in (("old", base | _lib.SC_PLAN_PLAIN_CACHE_POLICY), ("new", base)):
        plan = lib.plan_create([H, 256], [Mx, My], flags=flags)
        assert lib.plan_kernel_name(plan, 0) == "k_fft2d_fwd3"
        for mode in (_lib.SC_FWD_SCALED, _lib.SC_FWD_ADJ_C2R):
            for shift in (0, 1):                         # shift 1: the spectrum starts on an odd complex element
                buf, out = _guarded(ni * n, dev, shift)
                lib.transform_forward(plan, mode, x.data_ptr(), out.data_ptr(), ni, 0, _st())
                torch.cuda.synchronize()
                assert _guards_intact(buf, ni * n, shift)
                assert not torch.isnan(out).any()
                res[name, mode, shift] = out
            sb = torch.full((GUARD + P * ni * rows * My + GUARD, 2), float("nan"), device=dev)
            lib.transform_forward_sharded(plan, mode, x.data_ptr(), sb[GUARD:].data_ptr(), ni, sh, 0, _st())
            torch.cuda.synchronize()
            assert torch.isnan(sb[:GUARD]).all() and torch.isnan(sb[GUARD + P * ni * rows * My:]).all()
            res[name, mode, "sharded"] = sb[GUARD:GUARD + P * ni * rows * My]
        lib.plan_destroy(plan)
    for mode in (_lib.SC_FWD_SCALED, _lib.SC_FWD_ADJ_C2R):
        for key in (0, 1, "sharded"):
            assert torch.equal(res["new", mode, key].view(torch.int32), res["old", mode, key].view(torch.int32)), (mode, key)
        assert torch.equal(res["new", mode, 1], res["new", mode, 0])
        want = _to_shards(res["old", mode, 0].view(ni, Mx, My, 2), P, rows).view(-1, 2)
        assert torch.equal(res["new", mode, "sharded"], want)


# ---------------------------------------------------------------------------------------------- one layer step
def _fguard(n, dev):
    """(buffer, view of n floats) between two NaN bands of 2 * GUARD floats"""
    buf = torch.full((4 * GUARD + n,), float("nan"), device=dev)
    return buf, buf[2 * GUARD:2 * GUARD + n]


def _layer_step_guarded(lib, dev, x, w, bias, g, kept, flags):
    """sc_layer_forward + sc_layer_backward with y, xhat, gx, gW and gbias each between NaN guard bands"""
    from neuraloperator_amd.modes import kept_block
    B, Ci = x.shape[:2]
    Co = w.shape[1]
    spatial = list(x.shape[2:])
    kb, w_start = kept_block(spatial, list(kept), list(kept))
    assert list(kb) == list(kept)
    Mk = kept[0] * kept[1]
    plan = lib.plan_create(spatial, list(kept), flags=flags)
    try:
        L = lib.layer_desc(B, Ci, Co, list(w.shape[2:]), w_start)
        ws = torch.empty(lib.layer_workspace_bytes(plan, L), dtype=torch.uint8, device=dev)
        wv = torch.view_as_real(w.contiguous())
        bufs = {k: _fguard(n, dev) for k, n in (("y", B * Co * x[0, 0].numel()), ("xhat", 2 * B * Ci * Mk),
                                                ("gx", x.numel()), ("gw", wv.numel()), ("gbias", Co))}
        st = _st()
        lib.layer_forward(plan, L, x.data_ptr(), wv.data_ptr(), bias.reshape(-1).data_ptr(), bufs["y"][1].data_ptr(),
                          bufs["xhat"][1].data_ptr(), ws.data_ptr(), st)
        lib.layer_backward(plan, L, g.data_ptr(), bufs["xhat"][1].data_ptr(), wv.data_ptr(), bufs["gx"][1].data_ptr(),
                           bufs["gw"][1].data_ptr(), bufs["gbias"][1].data_ptr(), ws.data_ptr(), st)
        torch.cuda.synchronize()
    finally:
        lib.plan_destroy(plan)
    out = {}
    for k, (buf, view) in bufs.items():
        assert torch.isnan(buf[:2 * GUARD]).all() and torch.isnan(buf[2 * GUARD + view.numel():]).all(), k
        assert not torch.isnan(view).any(), k
        out[k] = view
    return out


def test_layer_step_new_default_against_restore_bit(lib, dev):
    """sc_layer_forward + sc_layer_backward at B = 32, C = 32, 64 x 64, modes 16: y, gx, gW, gbias and xhat.  Kept
    16 x 9 = 144 modes are 18 mode groups, not whole octets of workgroups, so this backward pass runs the bias gradient
    and two single contraction launches; the fused pair with its bias job is the next test."""
    B, C, S, m = 32, 32, 64, 16
    kept = [m, m // 2 + 1]
    torch.manual_seed(31)
    x, g = torch.randn(B, C, S, S, device=dev), torch.randn(B, C, S, S, device=dev)
    w = torch.randn(C, C, *kept, dtype=torch.cfloat, device=dev)
    bias = torch.randn(C, 1, 1, device=dev)
    assert lib.modegemm_pair_path(*_pair_descs(B, C, C, kept[0] * kept[1], _lib.SC_GEMM_STREAM_C, 0)) == 0
    old = layer_fwd_bwd(lib, x, w, bias, g, kept, kept, flags=_lib.SC_PLAN_PLAIN_CACHE_POLICY)
    new = layer_fwd_bwd(lib, x, w, bias, g, kept, kept, flags=0)
    for name, a, b in zip(("y", "gx", "gw", "gbias", "xhat"), new, old):
        assert not torch.isnan(torch.view_as_real(a) if a.is_complex() else a).any(), name
        assert torch.equal(a, b), name


@pytest.mark.parametrize("H", [64, 256])
def test_layer_step_with_the_fused_pair_and_its_bias_job(lib, dev, H):
    """A grid that takes k_fft2d_fwd3 (256 columns) with kept 16 x 8 = 128 modes: 16 mode groups, whole octets, so
    sc_layer_backward runs ONE k_modegemm_dma_bwd launch with the bias role in its trailing workgroups (asserted on the
    descriptors the layer builds).  New default (the transform stores xhat / ghat write-through) against the restore bit,
    every output between guard bands, bitwise.  The contraction sites of the policy are off in the product library and
    are not run here (tests/test_emu_cache_policy.py drives them through the measurement switch)."""
    B, C = 32, 32
    kept = [16, 8]
    Mk = kept[0] * kept[1]
    assert lib.modegemm_pair_path(*_pair_descs(B, C, C, Mk, _lib.SC_GEMM_STREAM_C, 0)) == 1
    torch.manual_seed(32)
    x, g = torch.randn(B, C, H, 256, device=dev), torch.randn(B, C, H, 256, device=dev)
    w = torch.randn(C, C, *kept, dtype=torch.cfloat, device=dev)
    bias = torch.randn(C, 1, 1, device=dev)
    old = _layer_step_guarded(lib, dev, x, w, bias, g, kept, _lib.SC_PLAN_PLAIN_CACHE_POLICY)
    new = _layer_step_guarded(lib, dev, x, w, bias, g, kept, 0)
    for name in old:
        assert torch.equal(new[name].view(torch.int32), old[name].view(torch.int32)), name


