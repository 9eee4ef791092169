// sc_kernels_wire.h -- the complex32 wire of the mode-parallel layer's half-precision exchanges.
//
// fno_block_precision "half" / "mixed" fixes the values at the points where the mode-parallel layer exchanges data:
// SC_GEMM_F16 rounds both operands to float16 when it reads them and rounds its result to float16
// (sc_kernels_generic.h, k_modegemm), in the forward contraction and in both gradient contractions.  So the four
// tensors that cross the all-to-all in a step (xhat, yhat, g_yhat, g_xhat) can travel as complex32 -- 4 bytes per mode
// instead of 8 -- without changing a value.  Two memory-bound kernels:
//
//   k_wire_pack_c32    complex64 spectrum [n][C][k1][rest] -> complex32 wire in the rank-major send layout
//                      [P][n][C][rows][rest]: kept row r lands on global row w0 + r of the P * rows concatenation
//                      (rank (w0 + r) / rows, local row (w0 + r) % rows), every other wire row is zero.  P = 1, w0 = 0,
//                      k1 = rows: a plain conversion.
//   k_wire_unpack_c32  the inverse gather: complex32 wire [P][n][C][rows][rest] -> complex64 rows [w0, w0 + k1) of the
//                      P * rows concatenation, [n][C][k1][rest].  P = 1, w0 = 0, k1 = rows: a plain conversion.
//
// Rounding is sc_round_f16 (nearest even; subnormals, overflow to inf and NaN as torch's cast).  A complex32 element is
// one 32-bit word, the real part in the low half (torch.complex32's layout).  A lane owns V consecutive elements of the
// OUTPUT (V = 2 when rows are even and the pointers aligned, else 1): lane l of a wave touches the V-element unit l of a
// run of 64, so every load and every store instruction covers contiguous bytes in lane order (V = 2: 16 B per lane on
// the complex64 side, 8 B on the wire side).  A row of `rest` elements is contiguous on both sides and V divides it, so
// a unit never straddles two rows.  WIRE_UNROLL units per lane are loaded before the first is stored.
#pragma once
#include "sc_device.h"

#define WIRE_UNROLL 4

struct alignas(8) wire_u2 {
  uint32_t x, y;
};

struct WireArgs {
  const void* src;
  void* dst;
  long long units;              // V-element units of the output
  long long rest;               // elements per row (the product of the mode dims after the first)
  long long nc;                 // n * C row blocks per rank block
  long long stride;             // grid stride in units
  int rows, k1, w0;             // wire rows per rank, spectrum rows, global wire row of spectrum row 0
};

// float16 bits of sc_round_f16(f) (exactly representable: the conversion below is exact)
#ifndef SC_EMU
SC_DEVICE uint32_t wire_f16_bits(const float f) { return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)sc_round_f16(f)); }
SC_DEVICE float wire_f16_value(const uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)h); }
#else
inline uint32_t wire_f16_bits(const float f) {
  const float r = sc_round_f16(f);
  uint32_t u;
  std::memcpy(&u, &r, 4);
  const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return sign | 0x7e00u | ((a >> 13) & 0x3ffu);     // NaN: quiet, payload truncated (v_cvt_f16_f32)
  if (a == 0x7f800000u) return sign | 0x7c00u;
  if (a >= 0x38800000u) return sign | (((a >> 23) - 112u) << 10) | ((a >> 13) & 0x3ffu);
  float m;
  std::memcpy(&m, &a, 4);
  return sign | (uint32_t)(m * 16777216.f);                               // subnormal: an integer multiple of 2^-24
}
inline float wire_f16_value(const uint32_t h) {
  const uint32_t sign = (h & 0x8000u) << 16, e = (h >> 10) & 0x1fu, m = h & 0x3ffu;
  uint32_t u;
  if (e == 0x1fu) {
    u = sign | 0x7f800000u | (m << 13) | (m ? 0x400000u : 0u);            // NaN: quiet (v_cvt_f32_f16)
  } else if (e) {
    u = sign | ((e + 112u) << 23) | (m << 13);
  } else {
    const float s = (float)m * (1.0f / 16777216.f);
    std::memcpy(&u, &s, 4);
    u |= sign;
  }
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
#endif

SC_DEVICE uint32_t wire_pack1(const float re, const float im) { return wire_f16_bits(re) | (wire_f16_bits(im) << 16); }

// element offset in the spectrum of wire element e, -1 for a zero row
SC_DEVICE long long wire_pack_src(const WireArgs& g, const long long e) {
  const long long row = e / g.rest, j = e - row * g.rest;
  const long long t = row / g.rows, lr = row - t * g.rows;
  const long long p = t / g.nc, slab = t - p * g.nc;
  const long long r = p * g.rows + lr - g.w0;
  return (r >= 0 && r < g.k1) ? (slab * g.k1 + r) * g.rest + j : -1;
}

// element offset in the wire of spectrum element e
SC_DEVICE long long wire_unpack_src(const WireArgs& g, const long long e) {
  const long long row = e / g.rest, j = e - row * g.rest;
  const long long slab = row / g.k1, r = row - slab * g.k1;
  const long long gr = g.w0 + r, p = gr / g.rows, lr = gr - p * g.rows;
  return ((p * g.nc + slab) * g.rows + lr) * g.rest + j;
}

template <int V>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_wire_pack_c32(WireArgs g) {
  for (long long u0 = (long long)SC_BID_X * (256 * WIRE_UNROLL) + SC_TID; u0 < g.units; u0 += g.stride) {
    if constexpr (V == 2) {
      const sc_f4* src = static_cast<const sc_f4*>(g.src);
      wire_u2* dst = static_cast<wire_u2*>(g.dst);
      sc_f4 v[WIRE_UNROLL];
#pragma unroll
      for (int k = 0; k < WIRE_UNROLL; ++k) {
        const long long u = u0 + k * 256;
        const long long s = u < g.units ? wire_pack_src(g, 2 * u) : -1;
        if (s >= 0) {
          v[k] = src[s >> 1];
        } else {
          v[k].x = v[k].y = v[k].z = v[k].w = 0.0f;
        }
      }
#pragma unroll
      for (int k = 0; k < WIRE_UNROLL; ++k) {
        const long long u = u0 + k * 256;
        if (u < g.units) {
          wire_u2 w;
          w.x = wire_pack1(v[k].x, v[k].y);
          w.y = wire_pack1(v[k].z, v[k].w);
          dst[u] = w;
        }
      }
    } else {
      const cf32* src = static_cast<const cf32*>(g.src);
      uint32_t* dst = static_cast<uint32_t*>(g.dst);
      cf32 v[WIRE_UNROLL];
#pragma unroll
      for (int k = 0; k < WIRE_UNROLL; ++k) {
        const long long u = u0 + k * 256;
        const long long s = u < g.units ? wire_pack_src(g, u) : -1;
        v[k] = s >= 0 ? src[s] : cf_make(0.0f, 0.0f);
      }
#pragma unroll
      for (int k = 0; k < WIRE_UNROLL; ++k) {
        const long long u = u0 + k * 256;
        if (u < g.units) dst[u] = wire_pack1(v[k].x, v[k].y);
      }
    }
  }
}

template <int V>
SC_GLOBAL void SC_LAUNCH_BOUNDS(256)
k_wire_unpack_c32(WireArgs g) {
  for (long long u0 = (long long)SC_BID_X * (256 * WIRE_UNROLL) + SC_TID; u0 < g.units; u0 += g.stride) {
    if constexpr (V == 2) {
      const wire_u2* src = static_cast<const wire_u2*>(g.src);
      sc_f4* dst = static_cast<sc_f4*>(g.dst);
      wire_u2 v[WIRE_UNROLL];
#pragma unroll
      for (int k = 0; k < WIRE_UNROLL; ++k) {
        const long long u = u0 + k * 256;
        if (u < g.units) v[k] = src[wire_unpack_src(g, 2 * u) >> 1];
      }
#pragma unroll
      for (int k = 0; k < WIRE_UNROLL; ++k) {
        const long long u = u0 + k * 256;
        if (u < g.units) {
          sc_f4 o;
          o.x = wire_f16_value(v[k].x & 0xffffu);
          o.y = wire_f16_value(v[k].x >> 16);
          o.z = wire_f16_value(v[k].y & 0xffffu);
          o.w = wire_f16_value(v[k].y >> 16);
          dst[u] = o;
        }
      }
    } else {
      const uint32_t* src = static_cast<const uint32_t*>(g.src);
      cf32* dst = static_cast<cf32*>(g.dst);
      uint32_t v[WIRE_UNROLL];
#pragma unroll
      for (int k = 0; k < WIRE_UNROLL; ++k) {
        const long long u = u0 + k * 256;
        if (u < g.units) v[k] = src[wire_unpack_src(g, u)];
      }
#pragma unroll
      for (int k = 0; k < WIRE_UNROLL; ++k) {
        const long long u = u0 + k * 256;
        if (u < g.units) dst[u] = cf_make(wire_f16_value(v[k] & 0xffffu), wire_f16_value(v[k] >> 16));
      }
    }
  }
}
