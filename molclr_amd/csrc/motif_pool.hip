// Motif readout: softmax-attention pool of gathered motif-embedding rows and
// the molecule's own feature row, forward in one launch and backward in two.
//
// Reference: models/ginet_finetune_mp.py:158-160, PyG 1.6.3's
// GlobalAttention(gate_nn = Linear(F, 1)) over cat(motif_embedding(clique_idx),
// h) by mol_idx.  There are B molecules; the T motif items of the batch are
// clique_idx [T] with mol_ptr [B + 1], so the rows of segment b are
//   x_i = E[clique_idx[i]],  i in [mol_ptr[b], mol_ptr[b + 1]),  then h[b] LAST
// (the reference appends the h rows after all motif rows, so its scatter_add
// adds them last).  gate g = x.w + c, alpha = exp(g - max_seg g) / sum_seg
// exp(g - max), a[b] = sum alpha_i x_i in that row order.  PyG adds 1e-16 to
// the segment sum; the sum contains exp(0) = 1 for the row that holds the
// max, so in fp32 1 + 1e-16 == 1 and the term is omitted here.
// At the reference's batch (32 molecules, ~10 rows of 512 floats per segment)
// that is ~15 launches of almost empty grids composed from torch ops.
//
// Forward (k_motif_fwd): one workgroup per molecule.  16 lanes share a row's
// gate: each walks the row in float4s (F % 4 == 0) or scalars, then a fixed
// xor tree; 16 rows are in flight per workgroup (4 waves, one per SIMD, eight
// independent 16-byte loads per lane at F = 512), which covers the L2 latency
// of a segment's ~20 KB in one round.  Every wave then takes the segment max
// and sum over the gates in the same fixed order (lane-strided, xor tree), the
// alphas are written, and each thread owns column chunks of a[b] and walks the
// rows in ascending order.  The per-row scalars sit in LDS for segments of up
// to kCap rows and in the alpha output itself for longer ones.
//
// Backward (a) (k_motif_bwd_seg): per molecule, with s_i = da.x_i and t = sum
// alpha_i s_i = da.a[b], dgate_i = alpha_i (s_i - t) is taken from s'_i =
// da.(x_i - a[b]), a dot product like the gates, as alpha_i (s'_i - u), u = sum
// alpha_i s'_i: the difference of two large dot products becomes a dot product
// of small differences (a segment whose weight sits on rows with large gates
// has x_i ~ a[b], and the rounding of s_i - t would reach dw through those
// large rows), and u takes out the rounding of a[b] that every s'_i carries,
// so that sum dgate_i = 0 holds to the rounding of the small terms.  dh[b] = alpha_h da +
// dgate_h w; the segment's share of dw and dc (sum dgate_i x_i, sum dgate_i,
// rows ascending) and the per-item dgate_i and molecule go to the workspace.
//
// Backward (b) (k_motif_bwd_params): one grid for dE, dw and dc.  The items
// arrive grouped by motif id (a stable sort of clique_idx: sorted ids and the
// permutation); the workgroup at the head of a run of equal ids walks the run
// -- ascending item order -- and writes dE[m] = sum alpha_i da[mol(i)] +
// dgate_i w, recomputed from the per-item scalars (no [T, F] scratch).  Rows
// of E without an item are zeroed by further workgroups that look each row up
// in the sorted ids (or left alone when the call accumulates).  dw and dc are
// the segments' shares summed over the molecules in ascending order.
//
// A clique_idx outside [0, num_motifs), or a mol_ptr that is not 0 = p_0 <=
// p_1 <= ... <= p_B = T, is never used as an index: it sets
// MOLCLR_STATUS_MOTIF_RANGE and makes that molecule's rows NaN.
//
// Plain fp32 fmaf everywhere, no floating-point atomics: results are
// bit-identical from run to run.
//
// Device-sized form (molclr_motif_pool_{fwd,bwd}_cap, for a captured step whose
// item count changes from replay to replay): the same kernels over an item
// CAPACITY T_cap.  T_cap sizes alpha ([T_cap + B], the h rows at T_cap + b),
// the grids and the workspace; the item count is read on the device as
// mol_ptr[B] (0 = p_0 <= ... <= p_B <= T_cap).  Items [p_B, T_cap) are padding:
// no segment holds them, and the dE pass skips them wherever the sort put them,
// so on the same items both forms run the same arithmetic in the same order.
#include "common.h"

#include <math.h>

namespace {

constexpr int kThreads = 256;  // 4 waves: 16 rows of a segment in flight
constexpr int kGroup = 16;     // lanes that share a row's dot product
constexpr int kGroups = kThreads / kGroup;
constexpr int kCap = 128;      // per-row scalars kept in LDS (longer: global)
constexpr int kZeroRows = 16;  // rows of E per zero-fill workgroup

struct PoolArgs {
  const float* h;
  const float* E;
  const int64_t* idx;
  const int32_t* ptr;
  const float* w;
  // T: the item capacity -- alpha's h rows start at T, grids and workspace are
  // sized by it.  The item count is T (dev_count 0) or ptr[B] (dev_count 1).
  int64_t B, T, num_motifs;
  int F;
  int dev_count;
};

// the item count; -1 for a device count outside [0, capacity]
__device__ __forceinline__ int64_t item_count(const int32_t* ptr, int64_t B, int64_t cap,
                                              int dev_count) {
  if (!dev_count) return cap;
  const int64_t t = ptr[B];
  return t >= 0 && t <= cap ? t : -1;
}

__device__ __forceinline__ float group_sum16(float v) {
  v += __shfl_xor(v, 8, kGroup);
  v += __shfl_xor(v, 4, kGroup);
  v += __shfl_xor(v, 2, kGroup);
  v += __shfl_xor(v, 1, kGroup);
  return v;
}

__device__ __forceinline__ float wave_sum64(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// number of motif items of molecule b, first item in p0; -1 for a mol_ptr
// that does not describe consecutive segments of [0, item count)
__device__ __forceinline__ int segment(const PoolArgs& p, int64_t b, int64_t& p0) {
  const int64_t lo = p.ptr[b], hi = p.ptr[b + 1];
  const int64_t t = item_count(p.ptr, p.B, p.T, p.dev_count);
  p0 = lo;
  const bool ok = t >= 0 && lo >= 0 && hi >= lo && hi <= t && (b > 0 || lo == 0) &&
                  (b < p.B - 1 || hi == t);
  return ok ? (int)(hi - lo) : -1;
}

// row i of segment b (i == n: the molecule's own h row); nullptr for a motif
// id outside the table
__device__ __forceinline__ const float* seg_row(const PoolArgs& p, int64_t b, int64_t p0, int n,
                                                int i) {
  if (i == n) return p.h + (size_t)b * p.F;
  const int64_t m = p.idx[p0 + i];
  if (m < 0 || m >= p.num_motifs) return nullptr;
  return p.E + (size_t)m * p.F;
}

// v.(x - sub) over the 16 lanes of a group (lane j of the group); sub may be null
template <bool VEC>
__device__ __forceinline__ float dot16(const float* __restrict__ x, const float* __restrict__ v,
                                       const float* __restrict__ sub, int F, int j) {
  float s = 0.f;
  if (VEC) {
    for (int k = 4 * j; k < F; k += 4 * kGroup) {
      float4 a = *reinterpret_cast<const float4*>(x + k);
      const float4 q = *reinterpret_cast<const float4*>(v + k);
      if (sub) {
        const float4 m = *reinterpret_cast<const float4*>(sub + k);
        a = make_float4(a.x - m.x, a.y - m.y, a.z - m.z, a.w - m.w);
      }
      s = fmaf(a.x, q.x, s);
      s = fmaf(a.y, q.y, s);
      s = fmaf(a.z, q.z, s);
      s = fmaf(a.w, q.w, s);
    }
  } else {
    for (int k = j; k < F; k += kGroup) s = fmaf(sub ? x[k] - sub[k] : x[k], v[k], s);
  }
  return group_sum16(s);
}

// sc[i] = (x_i - sub).v + add for the n + 1 rows of the segment, 16 rows at a time;
// returns through *bad whether a motif id was out of range (sc[i] = NaN there)
template <bool VEC>
__device__ __forceinline__ void row_dots(const PoolArgs& p, int64_t b, int64_t p0, int n,
                                         const float* __restrict__ v,
                                         const float* __restrict__ sub, float add, float* sc,
                                         int64_t h_slot, int* bad) {
  const int j = threadIdx.x % kGroup, group = threadIdx.x / kGroup;
  for (int i = group; i <= n; i += kGroups) {
    const float* x = seg_row(p, b, p0, n, i);
    float d;
    if (x) {
      d = dot16<VEC>(x, v, sub, p.F, j) + add;
    } else {
      d = __builtin_nanf("");
      if (j == 0) *bad = 1;
    }
    if (j == 0) sc[i == n ? h_slot : i] = d;
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_motif_fwd(const PoolArgs p, const float* __restrict__ c,
                                                        float* __restrict__ a, float* alpha,
                                                        int32_t* status) {
  __shared__ float s_sc[kCap];
  __shared__ int s_bad;
  const int64_t b = blockIdx.x;
  const int F = p.F;
  int64_t p0;
  const int n = segment(p, b, p0);
  float* arow = a + (size_t)b * F;
  if (n < 0) {  // nothing of this segment is an index
    if (threadIdx.x == 0 && status) atomicOr(status, MOLCLR_STATUS_MOTIF_RANGE);
    for (int k = threadIdx.x; k < F; k += kThreads) arow[k] = __builtin_nanf("");
    if (threadIdx.x == 0) alpha[p.T + b] = __builtin_nanf("");
    return;
  }
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  // the n + 1 per-row scalars: LDS, or the rows' alpha entries (items p0 ..
  // p0 + n - 1, then T + b) when the segment is longer than the LDS array
  const bool lds = n + 1 <= kCap;
  float* sc = lds ? s_sc : alpha + p0;
  const int64_t h_slot = lds ? n : p.T + b - p0;
  row_dots<VEC>(p, b, p0, n, p.w, nullptr, *c, sc, h_slot, &s_bad);
  __syncthreads();
  if (s_bad) {
    if (threadIdx.x == 0 && status) atomicOr(status, MOLCLR_STATUS_MOTIF_RANGE);
    for (int k = threadIdx.x; k < F; k += kThreads) arow[k] = __builtin_nanf("");
    for (int i = threadIdx.x; i <= n; i += kThreads)
      alpha[i == n ? p.T + b : p0 + i] = __builtin_nanf("");
    return;
  }
  // segment max and sum, the same fixed order in every wave
  const int lane = threadIdx.x & 63;
  float m = -INFINITY;
  for (int i = lane; i <= n; i += 64) m = fmaxf(m, sc[i == n ? h_slot : i]);
  m = wave_max(m);
  float s = 0.f;
  for (int i = lane; i <= n; i += 64) s += expf(sc[i == n ? h_slot : i] - m);
  s = wave_sum64(s);
  __syncthreads();  // every wave has read the gates
  for (int i = threadIdx.x; i <= n; i += kThreads) {
    const int64_t slot = i == n ? h_slot : i;
    const float al = expf(sc[slot] - m) / s;
    sc[slot] = al;
    alpha[i == n ? p.T + b : p0 + i] = al;
  }
  __syncthreads();
  // a[b] = sum_i alpha_i x_i: a thread owns column chunks, rows ascending
  const float* hrow = p.h + (size_t)b * F;
  if (VEC) {
    for (int k = 4 * threadIdx.x; k < F; k += 4 * kThreads) {
      float4 acc = f4zero();
#pragma unroll 4
      for (int i = 0; i < n; ++i) {
        const float4 x = *reinterpret_cast<const float4*>(p.E + (size_t)p.idx[p0 + i] * F + k);
        const float al = sc[i];
        acc.x = fmaf(al, x.x, acc.x);
        acc.y = fmaf(al, x.y, acc.y);
        acc.z = fmaf(al, x.z, acc.z);
        acc.w = fmaf(al, x.w, acc.w);
      }
      const float4 x = *reinterpret_cast<const float4*>(hrow + k);
      const float al = sc[h_slot];
      acc.x = fmaf(al, x.x, acc.x);
      acc.y = fmaf(al, x.y, acc.y);
      acc.z = fmaf(al, x.z, acc.z);
      acc.w = fmaf(al, x.w, acc.w);
      *reinterpret_cast<float4*>(arow + k) = acc;
    }
  } else {
    for (int k = threadIdx.x; k < F; k += kThreads) {
      float acc = 0.f;
#pragma unroll 4
      for (int i = 0; i < n; ++i) acc = fmaf(sc[i], p.E[(size_t)p.idx[p0 + i] * F + k], acc);
      arow[k] = fmaf(sc[h_slot], hrow[k], acc);
    }
  }
}

struct SegGrads {
  const float* da;
  const float* a;  // the forward's output
  const float* alpha;
  float* dh;      // nullable
  float* dgate;   // workspace [T + B]
  int32_t* mol;   // workspace [T]
  float* dwp;     // workspace [B, F], nullable (no dw wanted)
  float* dcp;     // workspace [B]
};

template <bool VEC>
__global__ __launch_bounds__(kThreads) void k_motif_bwd_seg(const PoolArgs p, const SegGrads g) {
  __shared__ float s_sc[kCap];
  __shared__ int s_bad;
  const int64_t b = blockIdx.x;
  const int F = p.F;
  int64_t p0;
  const int n = segment(p, b, p0);
  const float* darow = g.da + (size_t)b * F;
  const float nan = __builtin_nanf("");
  if (n < 0) {
    for (int k = threadIdx.x; k < F; k += kThreads) {
      if (g.dh) g.dh[(size_t)b * F + k] = nan;
      if (g.dwp) g.dwp[(size_t)b * F + k] = nan;
    }
    if (threadIdx.x == 0) g.dgate[p.T + b] = g.dcp[b] = nan;
    return;
  }
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  const bool lds = n + 1 <= kCap;
  float* sc = lds ? s_sc : g.dgate + p0;
  const int64_t h_slot = lds ? n : p.T + b - p0;
  // s_i - t = da.(x_i - a[b])
  row_dots<VEC>(p, b, p0, n, darow, g.a + (size_t)b * F, 0.f, sc, h_slot, &s_bad);
  __syncthreads();
  const bool bad = s_bad != 0;  // the forward made this molecule's alphas NaN
  const int lane = threadIdx.x & 63;
  // u = sum alpha_i s'_i is 0 but for the rounding of a[b], which all s'_i share
  float u = 0.f;
  for (int i = lane; i <= n; i += 64)
    u = fmaf(g.alpha[i == n ? p.T + b : p0 + i], sc[i == n ? h_slot : i], u);
  u = wave_sum64(u);
  __syncthreads();  // every wave has read the s'_i
  for (int i = threadIdx.x; i <= n; i += kThreads) {
    const int64_t slot = i == n ? h_slot : i, row = i == n ? p.T + b : p0 + i;
    const float dg = g.alpha[row] * (sc[slot] - u);
    sc[slot] = dg;
    g.dgate[row] = dg;
    if (i < n) g.mol[p0 + i] = (int32_t)b;
  }
  __syncthreads();
  if (threadIdx.x < 64) {  // the segment's share of dc, fixed order
    float s = 0.f;
    for (int i = lane; i <= n; i += 64) s += sc[i == n ? h_slot : i];
    s = wave_sum64(s);
    if (lane == 0) g.dcp[b] = s;
  }
  // dh[b] = alpha_h da + dgate_h w;  dwp[b] = sum_i dgate_i x_i, rows ascending
  const float al_h = g.alpha[p.T + b], dg_h = sc[h_slot];
  const float* hrow = p.h + (size_t)b * F;
  for (int k = threadIdx.x; k < F; k += kThreads) {
    if (g.dh) g.dh[(size_t)b * F + k] = fmaf(al_h, darow[k], dg_h * p.w[k]);
    if (!g.dwp) continue;
    float acc = 0.f;
    if (bad) {
      acc = nan;
    } else {
#pragma unroll 4
      for (int i = 0; i < n; ++i) acc = fmaf(sc[i], p.E[(size_t)p.idx[p0 + i] * F + k], acc);
      acc = fmaf(dg_h, hrow[k], acc);
    }
    g.dwp[(size_t)b * F + k] = acc;
  }
}

struct ParamGrads {
  const float* da;
  const float* alpha;
  const float* w;
  const int64_t* sorted;  // clique_idx in ascending order (stable)
  const int64_t* order;   // the item at each sorted position
  const float* dgate;
  const int32_t* mol;
  const float* dwp;
  const float* dcp;
  const int32_t* ptr;  // mol_ptr: the item count with dev_count
  float* dE;
  float* dw;
  float* dc;
  int acc_dE, acc_dw, acc_dc;
  int dev_count;
  int64_t B, T, num_motifs;  // T: the capacity, as PoolArgs
  int F;
  int64_t run_blocks, zero_blocks;  // then the dw / dc workgroups
};

__global__ __launch_bounds__(kThreads) void k_motif_bwd_params(const ParamGrads g) {
  const int F = g.F;
  int64_t blk = blockIdx.x;
  if (blk < g.run_blocks) {
    // the head of a run of equal motif ids sums the run into dE[m]
    const int64_t m = g.sorted[blk];
    if (blk > 0 && g.sorted[blk - 1] == m) return;
    if (m < 0 || m >= g.num_motifs) return;  // never an index
    // items at and past the count are padding: skipped wherever they sorted to
    int64_t count = item_count(g.ptr, g.B, g.T, g.dev_count);
    if (count < 0) count = 0;
    if (g.dev_count && g.acc_dE) {  // a row only padding names stays as it is
      bool real = false;
      for (int64_t q = blk; q < g.T && g.sorted[q] == m && !real; ++q)
        real = g.order[q] >= 0 && g.order[q] < count;
      if (!real) return;
    }
    float* out = g.dE + (size_t)m * F;
    for (int k = threadIdx.x; k < F; k += kThreads) {
      float acc = 0.f;
      const float wk = g.w[k];
      for (int64_t q = blk; q < g.T && g.sorted[q] == m; ++q) {
        const int64_t i = g.order[q];
        if (i < 0 || i >= count) continue;
        const int64_t mb = g.mol[i];
        if (mb < 0 || mb >= g.B) continue;  // an item no valid segment holds
        acc += fmaf(g.alpha[i], g.da[(size_t)mb * F + k], g.dgate[i] * wk);
      }
      out[k] = g.acc_dE ? out[k] + acc : acc;
    }
    return;
  }
  blk -= g.run_blocks;
  if (blk < g.zero_blocks) {
    // rows of E that no item uses: looked up in the sorted ids, then zeroed
    __shared__ int s_empty[kZeroRows];
    const int64_t m0 = blk * kZeroRows;
    if (threadIdx.x < kZeroRows) {
      const int64_t m = m0 + threadIdx.x;
      int64_t lo = 0, hi = g.T;  // first position with sorted >= m
      while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (g.sorted[mid] < m) lo = mid + 1; else hi = mid;
      }
      s_empty[threadIdx.x] = m < g.num_motifs && !(lo < g.T && g.sorted[lo] == m);
    }
    __syncthreads();
    for (int r = 0; r < kZeroRows; ++r) {
      if (!s_empty[r]) continue;
      float* out = g.dE + (size_t)(m0 + r) * F;
      for (int k = threadIdx.x; k < F; k += kThreads) out[k] = 0.f;
    }
    return;
  }
  blk -= g.zero_blocks;
  // dw = sum_b dwp[b], dc = sum_b dcp[b]: molecules ascending
  const int k = (int)blk * kThreads + threadIdx.x;
  if (g.dw && k < F) {
    float acc = 0.f;
#pragma unroll 4
    for (int64_t b = 0; b < g.B; ++b) acc += g.dwp[(size_t)b * F + k];
    g.dw[k] = g.acc_dw ? g.dw[k] + acc : acc;
  }
  if (g.dc && blk == 0 && threadIdx.x == 0) {
    float acc = 0.f;
    for (int64_t b = 0; b < g.B; ++b) acc += g.dcp[b];
    *g.dc = g.acc_dc ? *g.dc + acc : acc;
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int fill_args(PoolArgs& p, const float* h, const float* E, const int64_t* clique_idx,
              const int32_t* mol_ptr, const float* w, int64_t B, int64_t T, int64_t F,
              int64_t num_motifs, bool dev_count, const char* who) {
  MOLCLR_REQUIRE(B >= 1 && B < ((int64_t)1 << 31), "%s: %lld molecules (1 .. 2^31 - 1)", who,
                 (long long)B);
  MOLCLR_REQUIRE(T >= 0 && T < ((int64_t)1 << 31), "%s: %lld items (0 .. 2^31 - 1)", who,
                 (long long)T);
  MOLCLR_REQUIRE(F >= 1 && F < ((int64_t)1 << 24), "%s: width %lld (1 .. 2^24 - 1)", who,
                 (long long)F);
  MOLCLR_REQUIRE(num_motifs >= 0 && num_motifs < ((int64_t)1 << 31),
                 "%s: %lld motifs (0 .. 2^31 - 1)", who, (long long)num_motifs);
  MOLCLR_REQUIRE(h && w && mol_ptr, "%s: null h / gate weight / mol_ptr", who);
  MOLCLR_REQUIRE(T == 0 || (E && clique_idx), "%s: null embedding table / clique_idx", who);
  p.h = h;
  p.E = E;
  p.idx = clique_idx;
  p.ptr = mol_ptr;
  p.w = w;
  p.B = B;
  p.T = T;
  p.num_motifs = num_motifs;
  p.F = (int)F;
  p.dev_count = dev_count ? 1 : 0;
  return MOLCLR_OK;
}

size_t bwd_bytes(int64_t B, int64_t T, int64_t F) {
  // dgate [T + B], mol [T], dwp [B, F], dcp [B], each from a 256-byte boundary
  return molclr::align_up(sizeof(float) * (size_t)(T + B), 256) +
         molclr::align_up(sizeof(int32_t) * (size_t)T, 256) +
         molclr::align_up(sizeof(float) * (size_t)B * (size_t)F, 256) +
         molclr::align_up(sizeof(float) * (size_t)B, 256);
}

}  // namespace

MOLCLR_API size_t molclr_motif_pool_workspace_bytes(int64_t B, int64_t T, int64_t F) {
  if (B < 1 || T < 0 || F < 1) return 0;
  return bwd_bytes(B, T, F);
}

namespace {

// both forms: T is the item count (dev_count false) or the capacity
int pool_fwd(const float* h, const float* E, const int64_t* clique_idx, const int32_t* mol_ptr,
             const float* gate_weight, const float* gate_bias, int64_t B, int64_t T, int64_t F,
             int64_t num_motifs, float* a, float* alpha, int32_t* status, bool dev_count,
             molclr_stream_t stream, const char* who) {
  PoolArgs p;
  MOLCLR_TRY_RC(fill_args(p, h, E, clique_idx, mol_ptr, gate_weight, B, T, F, num_motifs,
                          dev_count, who));
  MOLCLR_REQUIRE(gate_bias && a && alpha, "%s: null gate bias / a / alpha", who);
  const bool vec = F % 4 == 0 && aligned16(h) && aligned16(E) && aligned16(gate_weight) && aligned16(a);
  hipStream_t s = molclr::as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(k_motif_fwd<true>, dim3((unsigned)B), dim3(kThreads), 0, s, p, gate_bias, a,
                       alpha, status);
  else
    hipLaunchKernelGGL(k_motif_fwd<false>, dim3((unsigned)B), dim3(kThreads), 0, s, p, gate_bias, a,
                       alpha, status);
  MOLCLR_LAUNCHED();
  return MOLCLR_OK;
}

int pool_bwd(const float* da, const float* h, const float* E, const int64_t* clique_idx,
             const int32_t* mol_ptr, const int64_t* sorted_idx, const int64_t* order,
             const float* gate_weight, const float* a, const float* alpha, int64_t B, int64_t T,
             int64_t F, int64_t num_motifs, float* dh, float* dE, float* dweight, float* dbias,
             int acc_dE, int acc_dweight, int acc_dbias, void* workspace, size_t workspace_bytes,
             bool dev_count, molclr_stream_t stream, const char* who) {
  PoolArgs p;
  MOLCLR_TRY_RC(fill_args(p, h, E, clique_idx, mol_ptr, gate_weight, B, T, F, num_motifs,
                          dev_count, who));
  MOLCLR_REQUIRE(da && a && alpha, "%s: null da / a / alpha", who);
  MOLCLR_REQUIRE(!dE || T == 0 || (sorted_idx && order),
                 "%s: dE needs the items sorted by motif id", who);
  MOLCLR_REQUIRE_WS(workspace_bytes, bwd_bytes(B, T, F));
  MOLCLR_REQUIRE(workspace, "%s: null workspace", who);
  molclr::Workspace ws(workspace, workspace_bytes);
  SegGrads g;
  g.da = da;
  g.a = a;
  g.alpha = alpha;
  g.dh = dh;
  g.dgate = ws.take<float>((size_t)(T + B));
  g.mol = ws.take<int32_t>((size_t)T);
  float* dwp = ws.take<float>((size_t)B * (size_t)F);
  g.dwp = dweight ? dwp : nullptr;
  g.dcp = ws.take<float>((size_t)B);
  if (!ws.ok()) {
    molclr::set_error("%s: workspace too small", who);
    return MOLCLR_ERR_WORKSPACE;
  }
  const bool vec = F % 4 == 0 && aligned16(h) && aligned16(E) && aligned16(da) && aligned16(a);
  hipStream_t s = molclr::as_stream(stream);
  if (vec)
    hipLaunchKernelGGL(k_motif_bwd_seg<true>, dim3((unsigned)B), dim3(kThreads), 0, s, p, g);
  else
    hipLaunchKernelGGL(k_motif_bwd_seg<false>, dim3((unsigned)B), dim3(kThreads), 0, s, p, g);
  MOLCLR_LAUNCHED();

  ParamGrads q;
  q.da = da;
  q.alpha = alpha;
  q.w = gate_weight;
  q.sorted = sorted_idx;
  q.order = order;
  q.dgate = g.dgate;
  q.mol = g.mol;
  q.dwp = dwp;
  q.dcp = g.dcp;
  q.ptr = mol_ptr;
  q.dev_count = p.dev_count;
  q.dE = dE;
  q.dw = dweight;
  q.dc = dbias;
  q.acc_dE = acc_dE;
  q.acc_dw = acc_dweight;
  q.acc_dc = acc_dbias;
  q.B = B;
  q.T = T;
  q.num_motifs = num_motifs;
  q.F = (int)F;
  q.run_blocks = dE ? T : 0;
  q.zero_blocks = dE && !acc_dE ? molclr::ceil_div(num_motifs, kZeroRows) : 0;
  const int64_t blocks = q.run_blocks + q.zero_blocks +
                         (dweight || dbias ? molclr::ceil_div(F, kThreads) : 0);
  MOLCLR_REQUIRE(blocks < ((int64_t)1 << 31), "%s: grid too large", who);
  if (blocks > 0) {
    hipLaunchKernelGGL(k_motif_bwd_params, dim3((unsigned)blocks), dim3(kThreads), 0, s, q);
    MOLCLR_LAUNCHED();
  }
  return MOLCLR_OK;
}

}  // namespace

MOLCLR_API int molclr_motif_pool_fwd(const float* h, const float* E, const int64_t* clique_idx,
                                     const int32_t* mol_ptr, const float* gate_weight,
                                     const float* gate_bias, int64_t B, int64_t T, int64_t F,
                                     int64_t num_motifs, float* a, float* alpha, int32_t* status,
                                     molclr_stream_t stream) {
  return pool_fwd(h, E, clique_idx, mol_ptr, gate_weight, gate_bias, B, T, F, num_motifs, a, alpha,
                  status, false, stream, "motif_pool_fwd");
}

MOLCLR_API int molclr_motif_pool_bwd(const float* da, const float* h, const float* E,
                                     const int64_t* clique_idx, const int32_t* mol_ptr,
                                     const int64_t* sorted_idx, const int64_t* order,
                                     const float* gate_weight, const float* a,
                                     const float* alpha, int64_t B, int64_t T, int64_t F,
                                     int64_t num_motifs, float* dh, float* dE,
                                     float* dweight, float* dbias, int acc_dE, int acc_dweight,
                                     int acc_dbias, void* workspace, size_t workspace_bytes,
                                     molclr_stream_t stream) {
  return pool_bwd(da, h, E, clique_idx, mol_ptr, sorted_idx, order, gate_weight, a, alpha, B, T, F,
                  num_motifs, dh, dE, dweight, dbias, acc_dE, acc_dweight, acc_dbias, workspace,
                  workspace_bytes, false, stream, "motif_pool_bwd");
}

MOLCLR_API size_t molclr_motif_pool_cap_workspace_bytes(int64_t B, int64_t T_cap, int64_t F) {
  return molclr_motif_pool_workspace_bytes(B, T_cap, F);
}

MOLCLR_API int molclr_motif_pool_fwd_cap(const float* h, const float* E, const int64_t* clique_idx,
                                         const int32_t* mol_ptr, const float* gate_weight,
                                         const float* gate_bias, int64_t B, int64_t T_cap,
                                         int64_t F, int64_t num_motifs, float* a, float* alpha,
                                         int32_t* status, molclr_stream_t stream) {
  return pool_fwd(h, E, clique_idx, mol_ptr, gate_weight, gate_bias, B, T_cap, F, num_motifs, a,
                  alpha, status, true, stream, "motif_pool_fwd_cap");
}

MOLCLR_API int molclr_motif_pool_bwd_cap(const float* da, const float* h, const float* E,
                                         const int64_t* clique_idx, const int32_t* mol_ptr,
                                         const int64_t* sorted_idx, const int64_t* order,
                                         const float* gate_weight, const float* a,
                                         const float* alpha, int64_t B, int64_t T_cap, int64_t F,
                                         int64_t num_motifs, float* dh, float* dE, float* dweight,
                                         float* dbias, int acc_dE, int acc_dweight, int acc_dbias,
                                         void* workspace, size_t workspace_bytes,
                                         molclr_stream_t stream) {
  return pool_bwd(da, h, E, clique_idx, mol_ptr, sorted_idx, order, gate_weight, a, alpha, B, T_cap,
                  F, num_motifs, dh, dE, dweight, dbias, acc_dE, acc_dweight, acc_dbias, workspace,
                  workspace_bytes, true, stream, "motif_pool_bwd_cap");
}
