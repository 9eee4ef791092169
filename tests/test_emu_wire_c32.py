"""CPU tier: the complex32 wire of the half-precision mode exchange (include/sc_engine.h sc_wire_pack_c32 /
sc_wire_unpack_c32, sc_kernels_wire.h) on the host-emulation build, bit for bit against a torch restatement: torch's
float32 -> float16 cast of the (real, imag) pairs, the kept rows placed on the P * rows wire rows (zero elsewhere),
rank-major; and the inverse gather of a row window.  Ties, subnormals, overflow, +-inf, NaN; ragged k1 (the last ranks
carry zero rows), w0 > 0, P in {1, 2, 3, 8}; odd and even row lengths (one / two elements per lane)."""
import numpy as np
import pytest
import torch

from engine_runner import emu_lib


@pytest.fixture(scope="module")
def lib():
    return emu_lib()


SPECIAL = np.array([0.0, -0.0, 65504.0, 65519.9, 65520.0, -65520.0, 1e9, -1e9, 5.96e-8, 2.98e-8, 2.99e-8, 8.94e-8,
                    6.1e-5, 6.09e-5, -3e-6, np.inf, -np.inf, np.nan, -np.nan], dtype=np.float32)


def _values(numel, seed):
    """fp32 values over the whole float16 range: random magnitudes 1e-9 .. 1e5, the mantissa ties of [1, 2) and the
    specials above, shuffled"""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(numel).astype(np.float32) * np.float32(10.0) ** rng.integers(-9, 6, numel).astype(np.float32)
    ties = np.float32(1.0) + np.arange(0, 64, dtype=np.float32) * np.float32(2.0 ** -11) + np.float32(2.0 ** -12)
    extra = np.concatenate([SPECIAL, ties, -ties * np.float32(2.0 ** -15)])
    k = min(numel, extra.size)
    idx = rng.choice(numel, k, replace=False)
    v[idx] = extra[:k]
    return torch.from_numpy(v)


def _spec(n, c, k1, rest, seed):
    v = _values(n * c * k1 * int(np.prod(rest)) * 2, seed)
    return torch.view_as_complex(v.reshape(n, c, k1, *rest, 2))


def pack_ref(spec, P, rows, w0):
    """torch restatement: (n, C, k1, *rest) complex64 -> (P, n, C, rows, *rest) int32 words of complex32"""
    n, c, k1 = spec.shape[:3]
    rest = list(spec.shape[3:])
    full = torch.zeros(n, c, P * rows, *rest, dtype=torch.complex64)
    full[:, :, w0:w0 + k1] = spec
    wire = full.reshape(n, c, P, rows, *rest).movedim(2, 0)
    halves = torch.view_as_real(wire).half().contiguous()                 # (..., 2) float16: real, imag
    return halves.view(torch.int32).squeeze(-1)


def unpack_ref(wire, k1, w0):
    """torch restatement: (P, n, C, rows, *rest) int32 words -> rows [w0, w0 + k1) of the P * rows concatenation"""
    P, n, c, rows = wire.shape[:4]
    rest = list(wire.shape[4:])
    halves = wire.contiguous().unsqueeze(-1).view(torch.float16)           # (..., 2)
    full = torch.view_as_complex(halves.float().contiguous()).movedim(0, 2).reshape(n, c, P * rows, *rest)
    return full[:, :, w0:w0 + k1]


def _pack(lib, spec, P, rows, w0):
    n, c, k1 = spec.shape[:3]
    rest = list(spec.shape[3:])
    out = torch.full((P, n, c, rows, *rest), 0x5a5a5a5a, dtype=torch.int32)     # every word must be written
    lib.wire_pack_c32(spec.data_ptr(), out.data_ptr(), n, c, k1, int(np.prod(rest)), P, rows, w0, 0)
    return out


def _unpack(lib, wire, k1, w0):
    P, n, c, rows = wire.shape[:4]
    rest = list(wire.shape[4:])
    out = torch.full((n, c, k1, *rest), float("nan"), dtype=torch.complex64)
    lib.wire_unpack_c32(wire.data_ptr(), out.data_ptr(), n, c, k1, int(np.prod(rest)), P, rows, w0, 0)
    return out


def _bits(t):
    return torch.view_as_real(t).contiguous().view(torch.int32)


def _same(got, ref):
    """bit for bit; a NaN only as a NaN (torch's own CPU float16 -> float32 paths disagree on NaN payloads and signs)"""
    g, r = torch.view_as_real(got), torch.view_as_real(ref)
    nan = torch.isnan(r)
    return torch.equal(torch.isnan(g), nan) and torch.equal(_bits(got)[~nan], _bits(ref)[~nan])


# (n, C, k1, rest, P, rows, w0): every rank's rows, ragged k1, a window that starts past row 0
CASES = [
    (2, 3, 8, (6,), 1, 8, 0),          # P = 1: the plain conversion
    (1, 2, 5, (7,), 1, 6, 1),          # P = 1 with a window, odd rows (one element per lane)
    (2, 3, 8, (6,), 2, 4, 0),
    (1, 4, 5, (3, 4), 2, 3, 0),        # 5 rows over 2 ranks of 3: one zero row on rank 1
    (2, 2, 5, (5,), 3, 2, 0),          # 5 rows over 3 ranks of 2: rank 2 gets one kept row and one zero row
    (2, 2, 4, (6,), 3, 3, 3),          # w0 > 0: rows 3..6 of 9 (runtime-reduced n_modes on the stored layout)
    (1, 3, 9, (5, 3), 8, 2, 0),        # 9 rows over 8 ranks of 2: ranks 5..7 carry zero rows only
    (1, 2, 6, (4, 5), 8, 4, 13),       # w0 > 0 across rank boundaries, 8 ranks
    (3, 2, 32, (17,), 8, 4, 0),        # a configs[3]-like row split, odd rest
    (1, 2, 32, (8, 17), 8, 4, 0),      # even rest: two elements per lane
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n{}c{}k{}r{}P{}rows{}w{}".format(*c[:3], "x".join(map(str, c[3])), *c[4:]))
def test_pack_is_torchs_cast_placed(lib, case):
    n, c, k1, rest, P, rows, w0 = case
    spec = _spec(n, c, k1, rest, seed=k1 * 31 + P)
    got = _pack(lib, spec, P, rows, w0)
    assert torch.equal(got, pack_ref(spec, P, rows, w0))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n{}c{}k{}r{}P{}rows{}w{}".format(*c[:3], "x".join(map(str, c[3])), *c[4:]))
def test_unpack_is_the_inverse_gather(lib, case):
    n, c, k1, rest, P, rows, w0 = case
    # random float16 patterns (signalling NaNs made quiet: the hardware conversion quiets them)
    rng = np.random.default_rng(k1 + 7 * P)
    h = rng.integers(0, 1 << 16, size=(P, n, c, rows, *rest, 2), dtype=np.int64).astype(np.uint16)
    snan = ((h & 0x7c00) == 0x7c00) & ((h & 0x03ff) != 0) & ((h & 0x0200) == 0)
    h[snan] = 0x7e00
    wire = torch.from_numpy(h.view(np.int16).copy()).view(torch.int32).squeeze(-1)
    got = _unpack(lib, wire, k1, w0)
    assert _same(got, unpack_ref(wire, k1, w0))


def test_every_float16_pattern_converts_back(lib):
    """the whole float16 code space (signalling NaNs aside) through one plain unpack: torch's float16 -> float32"""
    h = np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)
    snan = ((h & 0x7c00) == 0x7c00) & ((h & 0x03ff) != 0) & ((h & 0x0200) == 0)
    h = h[~snan]
    h = h[: h.size // 2 * 2]
    wire = torch.from_numpy(h.view(np.int16).copy()).view(torch.int32).reshape(1, 1, 1, 1, -1)
    got = _unpack(lib, wire, 1, 0)
    ref = torch.view_as_complex(wire.contiguous().view(torch.float16).float().reshape(1, 1, 1, -1, 2))
    assert _same(got, ref)


@pytest.mark.parametrize("P,rows,k1,w0", [(2, 4, 8, 0), (3, 2, 5, 0), (8, 2, 9, 0), (2, 5, 6, 2)])
def test_round_trip_is_the_float16_rounding(lib, P, rows, k1, w0):
    """unpack(pack(x)) over the same window = complex(float16(re), float16(im)); the other rows of the wire are zero"""
    spec = _spec(2, 3, k1, (4, 3), seed=P * 11 + k1)
    wire = _pack(lib, spec, P, rows, w0)
    back = _unpack(lib, wire, k1, w0)
    ref = torch.view_as_complex(torch.view_as_real(spec).half().float().contiguous())
    assert _same(back, ref)
    full = _unpack(lib, wire, P * rows, 0)
    outside = torch.cat([full[:, :, :w0], full[:, :, w0 + k1:]], 2)
    assert torch.equal(_bits(outside), torch.zeros_like(_bits(outside)))


def test_row_window_past_the_wire_is_refused(lib):
    spec = _spec(1, 1, 5, (2,), seed=0)
    out = torch.empty(2, 1, 1, 2, 2, dtype=torch.int32)
    from neuraloperator_amd._lib import EngineError
    with pytest.raises(EngineError):
        lib.wire_pack_c32(spec.data_ptr(), out.data_ptr(), 1, 1, 5, 2, 2, 2, 0, 0)    # 5 rows > 2 ranks x 2
