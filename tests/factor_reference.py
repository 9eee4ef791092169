"""Helper of the factorised-weight kernel tests (sc_kernels_tucker.h, sc_kernels_fmx.h, k_modegemm_msum of
sc_kernels_generic.h): the case tables both tiers run (tests/test_gpu_factor_kernels.py on the device,
tests/test_emu_tucker_modes.py and tests/test_emu_fmx.py in host emulation), the float64 references written out
without autograd, a mirror of the host's route rules so that every row can NAME the instantiation it reaches, and a
runner that drives the C-ABI on buffers between NaN guard bands.

Bounds.  Every output is held at the project's rel-L2 bar and, element by element, at

    |got - ref| <= gamma_N S,        gamma_N = N u / (1 - N u),  u = 2^-24,

S = the float64 sum over the contraction of (|Re a| + |Im a|)(|Re b| + |Im b|) -- NOT |c|: the matrix-core kernels form
a complex product from three real ones, Im C = P3 - P1 - P2 with P3 = (Re A + Im A)(Re B + Im B), and lose accuracy
relative to that sum.  N is counted in the kernel source (n_dot, n_red below) and stored next to each case by
tucker_counts / bfac_counts / msum_counts; for the two-stage products S and N are carried through the intermediate:
with tmp_hat = tmp + e1, |e1| <= gamma_a S_tmp and |tmp_hat|_1 <= (1 + 2 gamma_a) S_tmp the second stage adds
gamma_b (1 + 2 gamma_a) S, together at most gamma_(a + b + 1) S.

    n_dot(steps) = 2 (4 steps + 1) + 6 = 8 steps + 8
        one real product P_i of `steps` k steps of v_mfma_f32_16x16x4_f32 accumulates 4 steps terms: at most one rounding
        per accumulation and one for the product should the unit not fuse them -> theta_(4 steps + 1) on every term.  P3's
        operands Re +- Im are rounded once each (+ 2); Im C = (P3 - P1) - P2 rounds twice more.  Against S:
        |err Im C| <= gamma_(4 steps + 5) S + gamma_(4 steps + 3) (S1 + S2), S1 + S2 <= S -> gamma_(8 steps + 8) S;
        Re C = P1 - P2 is below that.  The vector kernels (cf_mac: two fused multiply-adds per term and component,
        2 K roundings over K terms) stay below the same count, so one N serves both routes.
    n_red(n, groups) = ceil(n / groups) + groups
        the fixed-order reductions (k_tucker_reduce and k_pmlp_reduce1 + k_tucker_scatter: 16 groups, k_fmx_reduce: 64):
        group g adds the partials g, g + groups, ... in order, one thread then adds the group sums in order.
"""
import os
import re

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "neuraloperator_amd", "csrc")

U = 2.0 ** -24
BAR_TUCKER_FWD, BAR_TUCKER_GRAD, BAR_FMX, BAR_SLOT = 2e-6, 5e-6, 2e-6, 1e-5
GUARD_ROWS = 16                     # one 16-row tile of the tensor in front of and behind every written buffer
GUARD_BITS = 0x7FC0DEAD             # a quiet NaN with a payload: the guard bands
BODY_BITS = 0x7FC00BAD              # another one: the buffer itself before the call
TUCKER_VECTOR = 1                   # sc_tucker_modes_path: the vector kernels
TUCKER_WG_CAP = 512                 # tucker_wgs (sc_engine.cpp)
LDS_EDGE = 150 * 1024               # tucker_use_mx: the padded backward layout must fit
TUCKER_FWD = {1: "k_tucker_modes_fwd_mx<4,3>", 2: "k_tucker_modes_fwd_mx<4,4>", 3: "k_tucker_modes_fwd_mx<16,3>",
              4: "k_tucker_modes_fwd_mx<16,4>"}
TUCKER_BWD = {1: "k_tucker_modes_bwd_mx<3,9,3,3,2>", 2: "k_tucker_modes_bwd_mx<16,16,4,4,4>"}
# Every code sc_tucker_modes_path can return.  10 f + b with b = 1 needs Rx Ry <= 768 and My <= 48, which is f = 1: the
# small backward kernel never meets another forward one.
TUCKER_PATHS = (0, TUCKER_VECTOR, 11, 12, 22, 32, 42)
BFAC_INSTANCES = ((9, 3), (9, 4), (16, 3), (16, 4))
MSUM_INSTANCES = ((16, 9, 3), (9, 16, 4), (16, 16, 4))
SLOT_TILES = ((2, 4), (4, 8))


def _constants():
    """the limits this file mirrors, as the sources state them: a changed constant fails here, at import"""
    with open(os.path.join(CSRC, "sc_engine.cpp")) as f:
        eng = f.read()
    with open(os.path.join(CSRC, "sc_kernels_fmx.h")) as f:
        fmx = f.read()
    with open(os.path.join(CSRC, "sc_kernels_tucker.h")) as f:
        tk = f.read()
    assert "<= 150 * 1024" in eng and "env > 0 ? env : 512" in eng
    assert re.search(r"^#define SC_PMLP_RED_GROUPS 16\b", eng, re.M)
    assert re.search(r"^#define SC_FMX_LDK 66\b", fmx, re.M) and re.search(r"^#define SC_FMX_LDR 66\b", fmx, re.M)
    assert re.search(r"^#define SC_FMX_RED_RG 64\b", fmx, re.M)
    assert re.search(r"^#define SC_TK_UY_PER_THREAD 4\b", tk, re.M) and "SC_SHARED cf32 red[16][17];" in tk


_constants()


def gamma(n):
    return n * U / (1.0 - n * U)


def n_dot(steps):
    return 8 * steps + 8


def n_red(n, groups):
    return -(-n // groups) + groups


def ksteps(k):
    return (k + 3) >> 2


def rel_l2(a, b):
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))


def abs1(z):
    """|Re z| + |Im z| in float64"""
    z = np.asarray(z, np.complex128)
    return np.abs(z.real) + np.abs(z.imag)


# ----------------------------------------------------------------------------------------------------------------------
# mirror of the host's route rules (sc_engine.cpp tucker_route / tkm_layout, sc_host_modegemm.h)
# ----------------------------------------------------------------------------------------------------------------------
def _ld_rows(n4):
    return (n4 + 2) | 2


def _ld_k(n4):
    return ((n4 + 15) & ~31) + 16


def tucker_layout_bytes(rx, ry, mx, my, bwd=True):
    """bytes of tkm_layout(...).total complex elements"""
    rx4, ry4, mx4, my4 = ((v + 3) & ~3 for v in (rx, ry, mx, my))
    ldx = _ld_k(rx4) if bwd else _ld_rows(rx4)
    ldy = ldc = _ld_rows(ry4)
    ldt = _ld_rows(my4) if bwd else _ld_k(my4)
    ldg = lds = _ld_rows(my4)
    total = mx4 * ldx + my4 * ldy + rx4 * ldc + rx4 * ldt
    if bwd:
        total += mx4 * ldg + rx4 * lds
    return 8 * total


def tucker_vector_bytes(rx, ry, mx, my):
    return 8 * (mx * rx + my * ry + rx * ry + rx * my + mx * my + rx * my)


def tucker_path(fg, rx, ry, mx, my):
    """what sc_tucker_modes_path must return, worked out from the rule (not from the library)"""
    if min(fg, rx, ry, mx, my) <= 0 or max(rx, ry, mx, my) > 64 or my * ry > 1024:
        return 0
    if tucker_layout_bytes(rx, ry, mx, my) > LDS_EDGE:
        return TUCKER_VECTOR if tucker_vector_bytes(rx, ry, mx, my) <= LDS_EDGE else 0
    few, y3 = rx * ry <= 1024, my <= 48
    f = (1 if y3 else 2) if few else (3 if y3 else 4)
    b = 1 if (rx * ry <= 768 and mx * my <= 2304 and rx <= 48 and my <= 48 and ry <= 32) else 2
    return 10 * f + b


def tucker_kernels(path):
    if path == TUCKER_VECTOR:
        return "k_tucker_modes_fwd", "k_tucker_modes_bwd"
    return TUCKER_FWD[path // 10], TUCKER_BWD[path % 10]


def bfac_instance(R, Q):
    return (9 if R <= 36 else 16, 3 if Q <= 48 else 4)


def bfac_eligible(R, Q, M):
    return 8 <= Q <= 64 and 4 <= R <= 64 and M >= 64


def msum_instance(P, Q):
    pa, pb = (P + 3) // 4, (Q + 3) // 4
    if pa <= 16 and pb <= 9 and Q <= 48:
        return (16, 9, 3)
    return (9, 16, 4) if pa <= 9 else (16, 16, 4)


def msum_eligible(P, Q, M):
    return 8 <= P <= 64 and 8 <= Q <= 64 and M >= 64


def slot_tile(P, Q):
    return (4, 8) if (P >= 16 and Q >= 8) else (2, 4)


def slot_count(P, Q, M):
    """msum_geometry: the number of mode splits = workspace slots of the slot form"""
    pt, qt = slot_tile(P, Q)
    n_mt = (M + 63) // 64
    return max(1, min(4096 // (-(-P // (4 * pt)) * -(-Q // qt)), n_mt))


def fmx_wgs(chunks, cap, cus):
    """fmx_wgs (sc_host_modegemm.h): equal rounds, rounded down to a multiple of the unit count when that costs the
    busiest workgroup at most one more chunk"""
    rounds = -(-chunks // cap)
    wgs = -(-chunks // rounds)
    m = (wgs // cus) * cus
    if m >= cus and m < wgs and -(-chunks // m) <= rounds + 1:
        wgs = m
    return wgs


def bfac_wgs(P, R, Q, M, cus):
    q4, r4 = (Q + 3) & ~3, (R + 3) & ~3
    lds = 8 * (q4 * _ld_rows(r4) + r4 * 66)
    return fmx_wgs(P * ((M + 63) // 64), cus * min(4, 160 * 1024 // lds), cus)


# ----------------------------------------------------------------------------------------------------------------------
# the tables
# ----------------------------------------------------------------------------------------------------------------------
def _tk(fg, rx, ry, mx, my, path, gpu_only=False, scaled=False, why=""):
    return dict(fg=fg, rx=rx, ry=ry, mx=mx, my=my, path=path, gpu_only=gpu_only, scaled=scaled, why=why)


# name -> (FG, Rx, Ry, Mx, My), the path code the row must reach.  gpu_only: too slow for the emulator.
TUCKER_CASES = {
    "unit": _tk(1, 1, 1, 1, 1, 11, why="(K + 3) >> 2 == 1 in every product"),
    "ragged": _tk(7, 3, 5, 6, 4, 11),
    # an extent of 1 beside larger ones: its reciprocal ceil(2^32 / 1) does not fit the 32 bits tkm_div multiplies by
    "one_rx": _tk(3, 1, 5, 6, 4, 11),
    "one_ry": _tk(3, 5, 1, 6, 4, 11),
    "one_mx": _tk(3, 5, 4, 1, 6, 11),
    "one_my": _tk(3, 5, 4, 6, 1, 11),
    "tile15": _tk(5, 15, 15, 15, 15, 11),
    "tile16": _tk(5, 16, 16, 16, 16, 11),
    "tile17": _tk(5, 17, 17, 17, 17, 11),
    "tile17_scaled": _tk(5, 17, 17, 17, 17, 11, scaled=True, why="columns of 2^10 and 2^-10 on the small kernels"),
    "tiles_37_19_63_33": _tk(3, 37, 19, 63, 33, 11),
    "bwd_all_at_limit": _tk(4, 48, 16, 48, 48, 11, why="Rx Ry = 768, Mx My = 2304, Rx = My = 48: still the small kernel"),
    "bwd_rxry_816": _tk(4, 48, 17, 48, 48, 12),
    "bwd_rxry_816_scaled": _tk(4, 48, 17, 48, 48, 12, scaled=True, why="columns of 2^10 and 2^-10 on the large backward"),
    "bwd_mxmy_2352": _tk(4, 48, 16, 49, 48, 12),
    "bwd_rx_49": _tk(4, 49, 15, 48, 47, 12, why="t_c = 4: every wave builds its own block of tmp"),
    "bwd_my_49": _tk(4, 48, 16, 47, 49, 22, why="also forward TY 3 -> 4"),
    "bwd_ry_32": _tk(4, 24, 32, 64, 32, 11),
    "bwd_ry_33": _tk(4, 23, 33, 64, 31, 12),
    "fwd_4_4": _tk(3, 64, 1, 64, 64, 22),
    "fwd_16_3_my_ry_1024": _tk(3, 64, 64, 64, 16, 32, why="My Ry = 1024, the SC_TK_UY_PER_THREAD limit"),
    "fwd_16_3_small_m": _tk(3, 64, 64, 16, 16, 32),
    "fwd_16_3_scaled": _tk(3, 64, 64, 16, 16, 32, scaled=True, why="columns of 2^10 and 2^-10 on <16,3>"),
    "fwd_16_4": _tk(3, 64, 20, 16, 51, 42, why="Rx Ry = 1280, My Ry = 1020, padded layout 92 864 B"),
    "fwd_16_4_scaled": _tk(3, 64, 20, 16, 51, 42, scaled=True, why="columns of 2^10 and 2^-10 on <16,4>"),
    "lds_147328": _tk(3, 64, 16, 64, 56, 22, why="the last layout under 150 KB: matrix cores"),
    "lds_147328_scaled": _tk(3, 64, 16, 64, 56, 22, scaled=True, why="columns of 2^10 and 2^-10 on <4,4>"),
    "vector_64_16_64_64": _tk(3, 64, 16, 64, 64, 1, why="Mx = 64 = the last tid >> 2 row, My Ry = 1024, ng = 4"),
    "vector_scaled": _tk(3, 64, 16, 64, 64, 1, scaled=True, why="columns of 2^10 and 2^-10 on the vector kernels"),
    "vector_64_12_64_64": _tk(3, 64, 12, 64, 64, 1),
    "vector_60_16_64_64": _tk(3, 60, 16, 64, 64, 1, why="ng = 256 / 60 = 4 with four idle threads"),
    "robin_fg1": _tk(1, 36, 19, 64, 33, 11),
    "robin_fg512": _tk(512, 36, 19, 64, 33, 11, gpu_only=True, why="one slice per workgroup at the cap"),
    "robin_fg513": _tk(513, 36, 19, 64, 33, 11, gpu_only=True, why="workgroup 0 walks two slices"),
    "robin_fg1030": _tk(1030, 36, 19, 64, 33, 11, gpu_only=True, why="six workgroups walk three slices"),
    "robin_fg513_vector": _tk(513, 64, 16, 64, 64, 1, gpu_only=True),
}
# refused: (FG, Rx, Ry, Mx, My)
TUCKER_REFUSED = {"mx_65": (3, 8, 8, 65, 8), "my_ry_1025": (3, 8, 25, 8, 41), "my_ry_1536": (3, 32, 32, 64, 48)}


def _bf(P, R, Q, M, transposed=False, conj=(0, 0), strided=False, scaled=False, gpu_only=False, path5=True, why=""):
    return dict(P=P, R=R, Q=Q, M=M, transposed=transposed, conj=conj, strided=strided, scaled=scaled, gpu_only=gpu_only,
                path5=path5, why=why)


_BFAC_M = (64, 65, 79, 80, 81, 127, 128, 129)     # a tail inside a 16-lane wave block, on its edge, a whole empty wave
BFAC_CASES = {}
for _i, (_r, _q) in enumerate((r, q) for r in (4, 36, 37, 64) for q in (8, 16, 17, 48, 49, 64)):
    # the grid R x Q; the mode counts and the storage order of B cycle over it (each M three times, each order twelve)
    BFAC_CASES["grid_R%d_Q%d_M%d" % (_r, _q, _BFAC_M[_i % 8])] = _bf(2, _r, _q, _BFAC_M[_i % 8], transposed=bool((_i // 8 + _i) & 1))
for _r, _q in ((36, 48), (36, 49), (37, 48), (37, 49)):                     # one row per instantiation, at its edge
    for _ca, _cb in ((0, 0), (0, 1), (1, 0), (1, 1)):
        BFAC_CASES["conj%d%d_R%d_Q%d" % (_ca, _cb, _r, _q)] = _bf(3, _r, _q, 81, conj=(_ca, _cb))
    BFAC_CASES["order_qr_R%d_Q%d" % (_r, _q)] = _bf(3, _r, _q, 127, transposed=True)
    BFAC_CASES["scaled_R%d_Q%d" % (_r, _q)] = _bf(3, _r, _q, 65, scaled=True, why="columns of 2^10 and 2^-10")
BFAC_CASES.update({
    "strided_slice_A": _bf(3, 12, 9, 96, strided=True),
    "chunks_P1056_uneven_rounds": _bf(1056, 4, 8, 64, gpu_only=True, why="1056 chunks on 512 workgroups, 32 walk three"),
    "chunks_P1025": _bf(1025, 4, 8, 64, gpu_only=True),
    "chunks_P1": _bf(1, 4, 8, 64, why="one workgroup"),
    "not5_Q7": _bf(2, 36, 7, 64, path5=False),
    "not5_R3": _bf(2, 3, 36, 64, path5=False),
    "not5_M63": _bf(2, 36, 36, 63, path5=False),
})
BFAC_UNEVEN = "chunks_P1056_uneven_rounds"


def _ms(P, R, Q, M, conj=(1, 0), c_layout="plain", scaled=False, gpu_only=False, atomic=False, wgs=None, why=""):
    return dict(P=P, R=R, Q=Q, M=M, conj=conj, c_layout=c_layout, scaled=scaled, gpu_only=gpu_only, atomic=atomic, wgs=wgs,
                why=why)


# mode-summed on the matrix cores (P, R, Q, M): sc_modegemm_msum_path == 1
MSUM_CASES = {
    "i1693_P64_Q36": _ms(64, 2, 36, 128, atomic=True),
    "i16164_P64_Q37": _ms(64, 2, 37, 128),
    "i9164_P36_Q49": _ms(36, 3, 49, 130, atomic=True),
    "i16164_P37_Q49": _ms(37, 3, 49, 130),
    "i1693_P8_Q8": _ms(8, 5, 8, 64, wgs="chunks", why="five chunks, five workgroups: every workgroup one chunk"),
    "i16164_P64_Q64_M129": _ms(64, 2, 64, 129),
    "i1693_scaled": _ms(64, 2, 36, 128, scaled=True, why="columns of 2^10 and 2^-10"),
    "i9164_scaled": _ms(36, 3, 49, 130, scaled=True, why="columns of 2^10 and 2^-10"),
    "i16164_scaled": _ms(37, 3, 49, 130, scaled=True, why="columns of 2^10 and 2^-10"),
    "conj_plain": _ms(36, 3, 49, 130, conj=(0, 0)),
    "conj_b": _ms(37, 3, 49, 130, conj=(0, 1)),
    "conj_ab": _ms(64, 2, 36, 128, conj=(1, 1)),
    "strided_c": _ms(17, 2, 15, 70, c_layout="padded", why="c_sp = Q + 3: the gap keeps its sentinel"),
    "transposed_c": _ms(15, 2, 17, 70, c_layout="transposed", why="c_sp = 1, c_sq = P + 2"),
    "chunks_1100": _ms(8, 1100, 8, 64, gpu_only=True, wgs="fewer", why="1100 chunks on 512 workgroups, 76 walk three"),
}
for _p in (15, 16, 17):
    for _q in (15, 16, 17):
        MSUM_CASES["tp_P%d_Q%d" % (_p, _q)] = _ms(_p, 2, _q, 70)
# the slot form of k_modegemm_msum + k_fmx_reduce: sc_modegemm_msum_path == 0
SLOT_CASES = {
    "P65_wide": _ms(65, 3, 36, 130, atomic=True),
    "Q7_narrow": _ms(16, 3, 7, 130),
    "M63_P15_narrow": _ms(15, 2, 9, 63),
    "M63_P16_wide": _ms(16, 2, 9, 63),
    "reduce_n1": _ms(6, 3, 5, 63, why="npc = 30: not a multiple of 16"),
    "reduce_n63": _ms(6, 3, 5, 64 * 63 - 1),
    "reduce_n64": _ms(6, 3, 5, 64 * 64),
    "reduce_n65": _ms(6, 3, 5, 64 * 64 + 1),
    "strided_c": _ms(6, 3, 5, 200, c_layout="padded"),
    "plain_conj": _ms(19, 2, 33, 60, conj=(0, 0)),
}
SLOT_REDUCE_N = {"reduce_n1": 1, "reduce_n63": 63, "reduce_n64": 64, "reduce_n65": 65}


def emu_rows(table):
    return sorted(n for n, c in table.items() if not c["gpu_only"])


# ----------------------------------------------------------------------------------------------------------------------
# inputs and float64 references
# ----------------------------------------------------------------------------------------------------------------------
def _randc(gen, *shape):
    return torch.complex(torch.randn(*shape, generator=gen), torch.randn(*shape, generator=gen))


def _scale_columns(t):
    """one huge and one tiny column, 2^10 and 2^-10 (exact in fp32): cancellation in P3 - P1 - P2 shows up"""
    t = t.clone()
    t[..., 0] *= 2.0 ** 10
    t[..., -1] *= 2.0 ** -10
    return t


def _seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % (2 ** 31)


def tucker_inputs(name):
    c = TUCKER_CASES[name]
    g = torch.Generator().manual_seed(_seed(name))
    core, ux = _randc(g, c["fg"], c["rx"], c["ry"]), _randc(g, c["mx"], c["rx"])
    uy, gt = _randc(g, c["my"], c["ry"]), _randc(g, c["fg"], c["mx"], c["my"])
    if c["scaled"] and c["rx"] > 1 and c["ry"] > 1:
        ux, uy = _scale_columns(ux), _scale_columns(uy)
    return core, ux, uy, gt


def tucker_counts(c, n_wg):
    """N per output: the two products of its chain, the carry and, for the factor gradients, the accumulation over the
    slices of a workgroup in the same accumulators and the reduction of the n_wg partials"""
    nsl = -(-c["fg"] // n_wg)
    return {"t": n_dot(ksteps(c["ry"])) + n_dot(ksteps(c["rx"])) + 1,
            "gcore": n_dot(ksteps(c["mx"])) + n_dot(ksteps(c["my"])) + 1,
            "gux": n_dot(ksteps(c["ry"])) + n_dot(nsl * ksteps(c["my"])) + 1 + n_red(n_wg, 16),
            "guy": n_dot(ksteps(c["mx"])) + n_dot(nsl * ksteps(c["rx"])) + 1 + n_red(n_wg, 16)}


_REF_CACHE = {}


def tucker_reference(name):
    """(ref, S) per output in float64, T = einsum('ncd,xc,yd->nxy') and its gradients for the cotangent gt:
        tmp[n, c, y] = sum_d core[n, c, d] uy[y, d]           t[n, x, y]  = sum_c ux[x, c] tmp[n, c, y]
        s[n, c, y]   = sum_x conj(ux[x, c]) gt[n, x, y]       gcore[n, c, d] = sum_y s[n, c, y] conj(uy[y, d])
        gux[x, c] = sum_{n, y} gt[n, x, y] conj(tmp[n, c, y])  guy[y, d] = sum_{n, c} s[n, c, y] conj(core[n, c, d])
    computed once per case and left unchanged"""
    if ("tk", name) in _REF_CACHE:
        return _REF_CACHE[("tk", name)]
    core, ux, uy, gt = (z.numpy().astype(np.complex128) for z in tucker_inputs(name))
    tmp = core @ uy.T
    s = ux.conj().T @ gt
    ref = {"t": ux @ tmp, "gcore": s @ uy.conj(),
           "gux": np.einsum("nxy,ncy->xc", gt, tmp.conj()), "guy": np.einsum("ncy,ncd->yd", s, core.conj())}
    a_core, a_ux, a_uy, a_gt = abs1(core), abs1(ux), abs1(uy), abs1(gt)
    s_tmp = a_core @ a_uy.T
    s_s = a_ux.T @ a_gt
    S = {"t": a_ux @ s_tmp, "gcore": s_s @ a_uy,
         "gux": np.einsum("nxy,ncy->xc", a_gt, s_tmp), "guy": np.einsum("ncy,ncd->yd", s_s, a_core)}
    for v in list(ref.values()) + list(S.values()):
        v.setflags(write=False)
    _REF_CACHE[("tk", name)] = (ref, S)
    return ref, S


def fmx_inputs(kind, name):
    """bfac: A (P, R, M) (a slice of a larger array when strided), B (R, Q); msum / slot: A as the transposed view of an
    (R, P, M) activation tensor, as the autograd of the chain passes it, B (R, Q, M)"""
    c = {"bfac": BFAC_CASES, "msum": MSUM_CASES, "slot": SLOT_CASES}[kind][name]
    g = torch.Generator().manual_seed(_seed(kind + name))
    P, R, Q, M = c["P"], c["R"], c["Q"], c["M"]
    if kind == "bfac":
        if c["strided"]:
            a = _randc(g, P, R + 2, M + 8)[:, 1:R + 1, 4:M + 4]
        else:
            a = _randc(g, P, R, M)
        b = _randc(g, R, Q)
        if c["scaled"]:
            b = _scale_columns(b.t().contiguous()).t().contiguous()        # along r: inside every dot product
        return a, b
    a = _randc(g, R, P, M).transpose(0, 1)
    b = _randc(g, R, Q, M)
    if c["scaled"]:
        b = _scale_columns(b)                                                # along m: inside every dot product
    return a, b


def fmx_reference(kind, name):
    if (kind, name) in _REF_CACHE:
        return _REF_CACHE[(kind, name)]
    c = {"bfac": BFAC_CASES, "msum": MSUM_CASES, "slot": SLOT_CASES}[kind][name]
    a, b = (z.numpy().astype(np.complex128) for z in fmx_inputs(kind, name))
    ca, cb = c["conj"]
    a, b = (a.conj() if ca else a), (b.conj() if cb else b)
    sub = "prm,rq->pqm" if kind == "bfac" else "prm,rqm->pq"
    ref, S = np.einsum(sub, a, b, optimize=True), np.einsum(sub, abs1(a), abs1(b), optimize=True)
    ref.setflags(write=False)
    S.setflags(write=False)
    _REF_CACHE[(kind, name)] = (ref, S)
    return ref, S


def bfac_counts(c):
    """one product over R; the eligibility rows (another kernel: two fused multiply-adds per term) stay below it"""
    return n_dot(ksteps(c["R"]))


def msum_counts(c, n_wg):
    """the chunks of a workgroup (16 k steps each) accumulate in the same accumulators, then k_fmx_reduce"""
    rounds = -(-(c["R"] * ((c["M"] + 63) // 64)) // n_wg)
    return n_dot(16 * rounds) + 1 + n_red(n_wg, 64)


def slot_counts(c, slots):
    """a lane: 2 fused multiply-adds per (mode tile, r) and component; 64 lanes added in order; k_fmx_reduce"""
    tiles = -(-((c["M"] + 63) // 64) // slots)
    return 2 * c["R"] * tiles + 64 + 1 + n_red(slots, 64)


# ----------------------------------------------------------------------------------------------------------------------
# guarded buffers and the checks
# ----------------------------------------------------------------------------------------------------------------------
class Guarded:
    """n floats between two bands of GUARD_ROWS rows of `row` floats, everything a NaN bit pattern before the call"""

    def __init__(self, n, row, device, body_bits=BODY_BITS):
        self.n, self.g = int(n), GUARD_ROWS * int(row)
        self.raw = torch.full((self.n + 2 * self.g,), GUARD_BITS, dtype=torch.int32, device=device)
        self.raw[self.g:self.g + self.n] = body_bits
        self.body_bits = body_bits

    @property
    def ptr(self):
        return self.raw.data_ptr() + 4 * self.g

    def floats(self):
        return self.raw[self.g:self.g + self.n].view(torch.float32)

    def complex(self, *shape):
        return torch.view_as_complex(self.floats().view(*shape, 2)).cpu()

    def guards_intact(self):
        return bool((self.raw[:self.g] == GUARD_BITS).all()) and bool((self.raw[self.g + self.n:] == GUARD_BITS).all())

    def untouched(self):
        return self.guards_intact() and bool((self.raw[self.g:self.g + self.n] == self.body_bits).all())


def _stream(device):
    return torch.cuda.current_stream().cuda_stream if device.type == "cuda" else 0


def _sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize()


def _p(t):
    return torch.view_as_real(t).data_ptr()


def check(label, got, ref, S, n, bar, elementwise=True):
    """finite everywhere, rel-L2 under the project's bar, every element inside gamma_n S -- and the float64 reference
    rounded to fp32 inside the same bound (asserted on the host for every case).  Returns (rel-L2, worst |err| / bound)."""
    got = np.asarray(got).astype(np.complex128)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    assert np.isfinite(got.real).all() and np.isfinite(got.imag).all(), label + ": an element was not written"
    bound = gamma(n) * S
    r32 = ref.astype(np.complex64).astype(np.complex128)
    assert (np.maximum(np.abs((r32 - ref).real), np.abs((r32 - ref).imag)) <= bound).all(), label + ": the bound is below fp32 itself"
    rel = rel_l2(got, ref)
    err = np.maximum(np.abs((got - ref).real), np.abs((got - ref).imag))
    ratio = float((err / np.maximum(bound, 1e-300)).max())
    print("%s: rel-L2 %.3e (bar %.0e)  N %d  worst |err| / (gamma_N S) %.4f" % (label, rel, bar, n, ratio))
    assert rel < bar, (label, rel, bar)
    if elementwise:
        i = np.unravel_index(int(np.argmax(err / np.maximum(bound, 1e-300))), err.shape)
        assert ratio <= 1.0, (label, "element", i, "err", float(err[i]), "bound", float(bound[i]), "N", n)
    return rel, ratio


def run_tucker(lib, name, device, inputs=None):
    """forward and backward of one row through the C-ABI on guarded buffers.  Returns (outputs, stats): outputs the four
    complex64 tensors (CPU), stats {tensor: (rel-L2, worst ratio)} -- None when `inputs` replaces the row's own."""
    c = TUCKER_CASES[name]
    dims = (c["fg"], c["rx"], c["ry"], c["mx"], c["my"])
    fg, rx, ry, mx, my = dims
    assert tucker_path(*dims) == c["path"], (name, "the table names path", c["path"], "the rule gives", tucker_path(*dims))
    assert lib.tucker_modes_supported(*dims) and lib.tucker_modes_path(*dims) == c["path"], (name, lib.tucker_modes_path(*dims))
    core, ux, uy, gt = (z.to(device).contiguous() for z in (inputs or tucker_inputs(name)))
    n_wg = min(fg, TUCKER_WG_CAP)
    np_ = 2 * (mx * rx + my * ry)
    nbytes = lib.tucker_modes_workspace_bytes(*dims)
    assert nbytes == (n_wg + 16) * np_ * 4 + 256
    t = Guarded(2 * fg * mx * my, 2 * my, device)
    gc = Guarded(2 * fg * rx * ry, 2 * ry, device)
    ga = Guarded(2 * mx * rx, 2 * rx, device)
    gb = Guarded(2 * my * ry, 2 * ry, device)
    ws = Guarded(nbytes // 4, np_, device, body_bits=-1)
    st = _stream(device)
    lib.tucker_modes_forward(*dims, _p(core), _p(ux), _p(uy), t.ptr, st)
    lib.tucker_modes_backward(*dims, _p(core), _p(ux), _p(uy), _p(gt), gc.ptr, ga.ptr, gb.ptr, ws.ptr, st)
    _sync(device)
    for key, buf in (("t", t), ("gcore", gc), ("gux", ga), ("guy", gb), ("workspace", ws)):
        assert buf.guards_intact(), "%s: a store outside %s" % (name, key)
    out = {"t": t.complex(fg, mx, my), "gcore": gc.complex(fg, rx, ry), "gux": ga.complex(mx, rx), "guy": gb.complex(my, ry)}
    if inputs is not None:
        return out, None
    ref, S = tucker_reference(name)
    N = tucker_counts(c, n_wg)
    stats = {k: check("tucker %s %s" % (name, k), out[k].numpy(), ref[k], S[k], N[k],
                      BAR_TUCKER_FWD if k == "t" else BAR_TUCKER_GRAD) for k in ("t", "gcore", "gux", "guy")}
    return out, stats


def run_tucker_refused(lib, name, device):
    """a refused shape: path and supported 0, no workspace, both calls raise and write nothing"""
    dims = TUCKER_REFUSED[name]
    fg, rx, ry, mx, my = dims
    assert tucker_path(*dims) == 0 and lib.tucker_modes_path(*dims) == 0 and not lib.tucker_modes_supported(*dims)
    assert lib.tucker_modes_workspace_bytes(*dims) == 0
    g = torch.Generator().manual_seed(5)
    core, ux, uy, gt = (z.to(device) for z in (_randc(g, fg, rx, ry), _randc(g, mx, rx), _randc(g, my, ry), _randc(g, fg, mx, my)))
    t, gc = Guarded(2 * fg * mx * my, 2 * my, device), Guarded(2 * fg * rx * ry, 2 * ry, device)
    ga, gb, ws = Guarded(2 * mx * rx, 2 * rx, device), Guarded(2 * my * ry, 2 * ry, device), Guarded(1 << 16, 64, device)
    raised = 0
    for call in (lambda: lib.tucker_modes_forward(*dims, _p(core), _p(ux), _p(uy), t.ptr, _stream(device)),
                 lambda: lib.tucker_modes_backward(*dims, _p(core), _p(ux), _p(uy), _p(gt), gc.ptr, ga.ptr, gb.ptr, ws.ptr,
                                                   _stream(device))):
        try:
            call()
        except Exception as e:                                                # _lib.EngineError with the engine's text
            assert "limits" in str(e), e
            raised += 1
    _sync(device)
    assert raised == 2
    assert all(b.untouched() for b in (t, gc, ga, gb, ws))


def bfac_kw(c, a):
    P, R, Q, M = c["P"], c["R"], c["Q"], c["M"]
    tr = c["transposed"]
    return dict(P=P, Q=Q, R=R, n_modes=M, a_sp=a.stride(0), a_sr=a.stride(1), a_sm=1, b_sm=0, conj_a=c["conj"][0],
                conj_b=c["conj"][1], b_sr=(1 if tr else Q), b_sq=(R if tr else 1), c_sp=Q * M, c_sq=M, c_sm=1)


def run_bfac(lib, name, device, cus=1, inputs=None):
    c = BFAC_CASES[name]
    P, R, Q, M = c["P"], c["R"], c["Q"], c["M"]
    a, b = inputs or fmx_inputs("bfac", name)
    if c["strided"]:                                     # a copy to another device would pack the slice: rebuild it there
        big = torch.full((P, R + 2, M + 8), float("nan"), dtype=torch.complex64, device=device)
        big[:, 1:R + 1, 4:M + 4] = a.to(device)
        a = big[:, 1:R + 1, 4:M + 4]
    else:
        a = a.contiguous().to(device)
    assert a.is_contiguous() != c["strided"]
    store = (b.t().contiguous() if c["transposed"] else b.contiguous()).to(device)
    kw = bfac_kw(c, a)
    assert bfac_eligible(R, Q, M) == c["path5"] and (lib.modegemm_path(**kw) == 5) == c["path5"], (name, lib.modegemm_path(**kw))
    if name == BFAC_UNEVEN and cus > 1:
        n_wg, chunks = bfac_wgs(P, R, Q, M, cus), P * ((M + 63) // 64)
        assert n_wg % cus == 0 and n_wg < chunks and chunks % n_wg != 0, (n_wg, chunks)       # the round-down branch
    out = Guarded(2 * P * Q * M, 2 * M, device)
    lib.modegemm(_p(a), _p(store), out.ptr, _stream(device), **kw)
    _sync(device)
    assert out.guards_intact(), name + ": a store outside C"
    got = out.complex(P, Q, M)
    if inputs is not None:
        return got, None
    ref, S = fmx_reference("bfac", name)
    return got, {"c": check("bfac %s" % name, got.numpy(), ref, S, bfac_counts(c), BAR_FMX)}


def msum_kw(c, a):
    P, R, Q, M = c["P"], c["R"], c["Q"], c["M"]
    c_sp, c_sq = {"plain": (Q, 1), "padded": (Q + 3, 1), "transposed": (1, P + 2)}[c["c_layout"]]
    return dict(P=P, Q=Q, R=R, n_modes=M, a_sp=a.stride(0), a_sr=a.stride(1), a_sm=1, b_sr=Q * M, b_sq=M, b_sm=1,
                conj_a=c["conj"][0], conj_b=c["conj"][1], c_sp=c_sp, c_sq=c_sq, c_sm=0)


def run_msum(lib, kind, name, device, inputs=None):
    """sc_modegemm_msum_ws on a guarded C (strided layouts: the gaps are part of the check) and a guarded workspace
    pre-filled with 0xFF: every partial must be written.  kind 'msum' = the matrix-core kernel, 'slot' = the slot form."""
    c = (MSUM_CASES if kind == "msum" else SLOT_CASES)[name]
    P, R, Q, M = c["P"], c["R"], c["Q"], c["M"]
    a, b = inputs or fmx_inputs(kind, name)
    act = a.transpose(0, 1).contiguous().to(device)                          # (R, P, M): a is its transposed view
    a, b = act.transpose(0, 1), b.contiguous().to(device)
    kw = msum_kw(c, a)
    mx = kind == "msum"
    assert msum_eligible(P, Q, M) == mx and lib.modegemm_msum_path(**kw) == int(mx), (name, lib.modegemm_msum_path(**kw))
    nbytes = lib.modegemm_msum_workspace_bytes(**kw)
    assert nbytes > 256 and (nbytes - 256) % (8 * P * Q) == 0
    n_part = (nbytes - 256) // (8 * P * Q)
    chunks = R * ((M + 63) // 64)
    if mx:
        assert 1 <= n_part <= chunks
        if device.type == "cuda" and c["wgs"] == "chunks":
            assert n_part == chunks
        if device.type == "cuda" and c["wgs"] == "fewer":
            assert chunks >= 1100 and n_part < chunks and chunks % n_part != 0
        n = msum_counts(c, n_part)
    else:
        assert n_part == slot_count(P, Q, M) and SLOT_REDUCE_N.get(name, n_part) == n_part, (name, n_part)
        n = slot_counts(c, n_part)
    rows, cols = {"plain": (P, Q), "padded": (P, Q + 3), "transposed": (Q, P + 2)}[c["c_layout"]]
    out = Guarded(2 * rows * cols, 2 * cols, device)
    ws = Guarded(nbytes // 4, 2 * Q, device, body_bits=-1)
    lib.modegemm_msum_ws(_p(act), _p(b), out.ptr, ws.ptr, nbytes, _stream(device), **kw)
    _sync(device)
    assert out.guards_intact() and ws.guards_intact(), name + ": a store outside C or the workspace"
    part = ws.raw[ws.g:ws.g + ws.n].cpu()
    skip = (-ws.ptr % 256) // 4                                               # the engine aligns the partials to 256 bytes
    assert bool((part[skip:skip + 2 * n_part * P * Q] != -1).all()), name + ": a partial was not written"
    full = out.raw[out.g:out.g + out.n].cpu().view(rows, cols, 2)
    if c["c_layout"] == "padded":
        assert bool((full[:, Q:] == BODY_BITS).all()), name + ": a store into the gap of a strided C"
        got = torch.view_as_complex(full[:, :Q].contiguous().view(torch.float32))
    elif c["c_layout"] == "transposed":
        assert bool((full[:, P:] == BODY_BITS).all()), name + ": a store into the gap of a strided C"
        got = torch.view_as_complex(full[:, :P].contiguous().view(torch.float32)).t()
    else:
        got = torch.view_as_complex(full.contiguous().view(torch.float32))
    if inputs is not None:
        return got, None
    ref, S = fmx_reference(kind, name)
    stats = {"c": check("%s %s" % (kind, name), got.numpy(), ref, S, n, BAR_FMX if mx else BAR_SLOT)}
    if c["atomic"]:                                                           # the atomic form: arrival order, 1e-5 only
        c0 = torch.zeros(P, Q, dtype=torch.complex64, device=device)
        plain = dict(kw, c_sp=Q, c_sq=1)
        lib.modegemm_msum(_p(act), _p(b), _p(c0), _stream(device), **plain)
        _sync(device)
        rel = rel_l2(c0.cpu().numpy(), ref)
        print("%s %s atomic form: rel-L2 %.3e (bar %.0e)" % (kind, name, rel, BAR_SLOT))
        assert rel < BAR_SLOT, (name, rel)
    return got, stats


def kernel_labels(kind, name):
    """the kernels a row runs, for the worst-ratio report"""
    if kind == "tucker":
        f, b = tucker_kernels(TUCKER_CASES[name]["path"])
        return {"t": f, "gcore": b, "gux": b, "guy": b}
    if kind == "bfac":
        c = BFAC_CASES[name]
        return {"c": "k_modegemm_bfac_mx<%d,%d>" % bfac_instance(c["R"], c["Q"]) if c["path5"] else "not path 5"}
    if kind == "msum":
        c = MSUM_CASES[name]
        return {"c": "k_modegemm_msum_mx<%d,%d,%d>" % msum_instance(c["P"], c["Q"])}
    c = SLOT_CASES[name]
    return {"c": "k_modegemm_msum<%d,%d> slots" % slot_tile(c["P"], c["Q"])}


# ----------------------------------------------------------------------------------------------------------------------
# coverage: every route has a row, in the whole table and among the rows the emulator runs
# ----------------------------------------------------------------------------------------------------------------------
def coverage(emu_only=False):
    """{what: rows that name it}; raises if a path code, an instantiation or a slot tile has no row"""
    keep = (lambda c: not c["gpu_only"]) if emu_only else (lambda c: True)
    cov = {("tucker", p): [] for p in TUCKER_PATHS}
    cov.update({("bfac", i): [] for i in BFAC_INSTANCES})
    cov.update({("msum", i): [] for i in MSUM_INSTANCES})
    cov.update({("slot", i): [] for i in SLOT_TILES})
    for n, dims in TUCKER_REFUSED.items():
        cov[("tucker", tucker_path(*dims))].append(n)
    for n, c in TUCKER_CASES.items():
        if keep(c):
            cov[("tucker", c["path"])].append(n)
    for n, c in BFAC_CASES.items():
        if keep(c) and c["path5"]:
            cov[("bfac", bfac_instance(c["R"], c["Q"]))].append(n)
    for n, c in MSUM_CASES.items():
        if keep(c):
            cov[("msum", msum_instance(c["P"], c["Q"]))].append(n)
    for n, c in SLOT_CASES.items():
        if keep(c):
            cov[("slot", slot_tile(c["P"], c["Q"]))].append(n)
    missing = [k for k, rows in cov.items() if not rows]
    assert not missing, "no row reaches %s" % (missing,)
    return cov


coverage()
coverage(emu_only=True)
