// Dropout after the BatchNorms (models/ginet_molclr.py:107-111,
// models/gcn_molclr.py:147-151: F.dropout(h, drop_ratio, training)) as a
// counter-based mask: a pure function of (seed, call, layer, row, column), so
// every kernel that needs an element's mask -- the apply that stores h, the
// aggregation that applies the BatchNorm to its source rows, the BatchNorm
// backward -- recomputes it instead of reading a stored one.
//
// Stream definition.  Philox4x32-10 (Salmon et al., Random123; multipliers
// 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85).  One call
// covers one float4 column unit:
//   counter = (row, c = column / 4, layer, call_lo)
//   key     = (seed_lo, seed_hi ^ call_hi)
// and output word j belongs to column 4 c + j.  An element is kept iff
// word >= thr, thr = (uint32_t)(p * 2^32); kept elements are multiplied by
// scale = 1 / (1 - p), dropped ones are exactly 0.  `row` is the row of the
// graph the executor sees (the union of both views in a paired pass).
#pragma once

#include <stdint.h>

#include <hip/hip_runtime.h>

// Kernels take the dropout as a compile-time variant: NoDrop compiles to the
// code without it.
struct NoDrop {
  static constexpr bool kOn = false;
};
struct DropArgs {
  static constexpr bool kOn = true;
  const int64_t* key;  // device [2]: seed, call counter (molclr_dropout_next_key's key_out)
  uint32_t thr;        // (uint32_t)(p * 2^32)
  float scale;         // 1 / (1 - p)
  int32_t layer;
};

// host: the arguments of one layer's dropout, 0 <= p < 1
inline DropArgs make_drop_args(const int64_t* key, double p, int layer) {
  return DropArgs{key, (uint32_t)(p * 4294967296.0), 1.0f / (1.0f - (float)p), layer};
}

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// A thread's view of the dropout: the key read once, then one Philox call per
// column unit.  operator() maps a unit of BatchNorm(+ReLU) outputs to the
// dropped unit -- and, the map being linear, a unit of incoming gradients to
// the gradients behind the dropout.
template <typename DR>
struct Drop {
  __device__ __forceinline__ explicit Drop(const DR&) {}
  __device__ __forceinline__ float4 operator()(float4 v, int64_t, int) const { return v; }
};
template <>
struct Drop<DropArgs> {
  uint32_t k0, k1, call, layer, thr;
  float scale;
  __device__ __forceinline__ explicit Drop(const DropArgs& a) {
    const uint64_t seed = (uint64_t)a.key[0], n = (uint64_t)a.key[1];
    k0 = (uint32_t)seed;
    k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(n >> 32);
    call = (uint32_t)n;
    layer = (uint32_t)a.layer;
    thr = a.thr;
    scale = a.scale;
  }
  __device__ __forceinline__ uint4 words(int64_t row, int c) const {
    return philox4x32_10(make_uint4((uint32_t)row, (uint32_t)c, layer, call), k0, k1);
  }
  __device__ __forceinline__ float4 operator()(float4 v, int64_t row, int c) const {
    const uint4 w = words(row, c);
    return make_float4(w.x >= thr ? v.x * scale : 0.f, w.y >= thr ? v.y * scale : 0.f,
                       w.z >= thr ? v.z * scale : 0.f, w.w >= thr ? v.w * scale : 0.f);
  }
};
