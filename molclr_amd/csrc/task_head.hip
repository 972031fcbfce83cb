// Supervised task head: a small-batch chain of Linears with activations and
// the loss, forward in one launch and backward in two.
//
// Reference: the fine-tuning models' readout after the pooling
// (models/ginet_finetune.py:95-127,145-147, models/gcn_finetune.py:131-144,
// 162-164): feat_lin, then pred_head / pred_lin = Linear -> Softplus | ReLU ->
// ... -> Linear, and finetune.py:71-77's criterion (CrossEntropyLoss, MSELoss
// or L1Loss) on the prediction.  The reference batch is 32 molecules
// (config_finetune.yaml): composed from row-tiled GEMMs and element-wise ops
// that is ~25 launches of almost empty grids per step.
//
// Forward (k_head_fwd): rows are independent through the whole chain, so a
// workgroup takes kRows rows through all L layers.  The block's activations
// ping-pong between two LDS buffers; every a_l also goes to caller memory (the
// backward reads them, a_1 and a_L are outputs).  The weights are read through
// L2: 16 lanes share an output column, each walking the weight row in float4s
// (K % 4 == 0) or scalars, four columns per lane group so an activation read
// from LDS feeds four products, then a fixed xor tree over the 16 lanes.  The
// per-row loss goes to the workspace; the last workgroup to finish (an integer
// ticket) sums the rows in a fixed order and writes the mean.
//
// Backward (a) (k_head_bwd_delta): row-blocked like the forward.  delta_L from
// the loss (recomputed from the saved prediction) times *gloss, then
// delta_l = (delta_{l+1} W_{l+1} [+ dh at a_1]) * act_l'(a_l) down to dx; a
// thread owns an input column k and walks the weight's rows (coalesced over
// k), delta rows broadcast from LDS.  Every delta_l goes to the workspace.
//
// Backward (b) (k_head_bwd_wgrad): dW_l = delta_l^T a_{l-1} and db_l = sum_rows
// delta_l of every layer in one grid, 8 x 256 output tiles, each element summed
// over the rows in ascending order.
//
// Plain fp32 fmaf everywhere, no floating-point atomics: results are
// bit-identical from run to run.
#include "common.h"

#include <math.h>

namespace {

static_assert(2 * 4 * MOLCLR_TASK_HEAD_MAX_DIM * sizeof(float) + 64 <= 65536, "LDS row block");

constexpr int kMaxL = MOLCLR_TASK_HEAD_MAX_LAYERS;
constexpr int kRows = 4;       // rows per workgroup (forward and backward (a))
constexpr int kThreads = 512;  // 8 waves: two per SIMD to cover the L2 latency
constexpr int kGroup = 16;     // lanes that share an output column (forward)
constexpr int kCols = 4;       // output columns per lane group and pass
// two kRows x dim fp32 LDS buffers (65,408 B at the limit) and the kernels' few
// static words within the 64 KiB a workgroup gets without opting in to more
constexpr int kMaxDim = MOLCLR_TASK_HEAD_MAX_DIM;
constexpr int kWgN = 8;        // dW tile: output rows n
constexpr int kWgK = 256;      // dW tile: output columns k (one per thread)

struct HeadArgs {
  int L, loss;
  int64_t B;
  int dims[kMaxL + 1];
  int act[kMaxL];
  const float* x;
  int64_t ldx;
  const float* W[kMaxL];
  const float* b[kMaxL];
  float* a[kMaxL];
  const void* target;
  float* loss_out;
  int32_t* status;
  float* rowloss;
  int32_t* sync;
  int ld;  // LDS row stride (floats, a multiple of 4)
};

struct GradArgs {
  const float* gloss;
  const float* dh;
  const float* dpred;
  float* dx;
  int64_t lddx;
  float* delta[kMaxL];  // workspace, [B, dims[l + 1]]
  float* dW[kMaxL];
  float* db[kMaxL];
  int acc[kMaxL];
  int tile0[kMaxL + 1];  // first tile of each layer in launch (b)
};

// nn.Softplus(beta = 1, threshold = 20): z above the threshold, else
// log1p(exp(z)); exp(z) <= e^20 there, so nothing overflows
__device__ __forceinline__ float act_fwd(float z, int act) {
  if (act == MOLCLR_ACT_RELU) return z > 0.f ? z : 0.f;
  if (act == MOLCLR_ACT_SOFTPLUS) return z > 20.f ? z : log1pf(expf(z));
  return z;
}

// act'(z) from the saved a = act(z).  Softplus: sigmoid(z) = 1 - exp(-a) =
// -expm1(-a): a ~ e^z for very negative z (no cancellation at z = -100), and
// 1 - 2e-9 rounds to 1 at z = 19.99 as above the threshold
__device__ __forceinline__ float act_bwd(float a, int act) {
  if (act == MOLCLR_ACT_RELU) return a > 0.f ? 1.f : 0.f;
  if (act == MOLCLR_ACT_SOFTPLUS) return -expm1f(-a);
  return 1.f;
}

__device__ __forceinline__ float group_sum16(float v) {
  v += __shfl_xor(v, 8, kGroup);
  v += __shfl_xor(v, 4, kGroup);
  v += __shfl_xor(v, 2, kGroup);
  v += __shfl_xor(v, 1, kGroup);
  return v;
}

__device__ __forceinline__ float agent_load(const float* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// out[r][n] = act(sum_k in[r][k] W[n][k] + b[n]) for the block's kRows rows
template <bool VEC>
__device__ __forceinline__ void layer_fwd(const float* __restrict__ W, const float* __restrict__ b,
                                          const float* in, float* out, float* __restrict__ A,
                                          int K, int N, int act, int ld, int64_t row0,
                                          int64_t B) {
  const int j = threadIdx.x % kGroup;
  const int group = threadIdx.x / kGroup;
  for (int nb = group * kCols; nb < N; nb += (kThreads / kGroup) * kCols) {
    float acc[kRows][kCols];
#pragma unroll
    for (int r = 0; r < kRows; ++r)
#pragma unroll
      for (int c = 0; c < kCols; ++c) acc[r][c] = 0.f;
    const float* wrow[kCols];
#pragma unroll
    for (int c = 0; c < kCols; ++c) wrow[c] = W + (size_t)min(nb + c, N - 1) * K;
    if (VEC) {
      for (int k = 4 * j; k < K; k += 4 * kGroup) {
        float4 w[kCols], av[kRows];
#pragma unroll
        for (int c = 0; c < kCols; ++c) w[c] = *reinterpret_cast<const float4*>(wrow[c] + k);
#pragma unroll
        for (int r = 0; r < kRows; ++r) av[r] = *reinterpret_cast<const float4*>(in + r * ld + k);
#pragma unroll
        for (int r = 0; r < kRows; ++r)
#pragma unroll
          for (int c = 0; c < kCols; ++c) {
            float s = acc[r][c];
            s = fmaf(av[r].x, w[c].x, s);
            s = fmaf(av[r].y, w[c].y, s);
            s = fmaf(av[r].z, w[c].z, s);
            s = fmaf(av[r].w, w[c].w, s);
            acc[r][c] = s;
          }
      }
    } else {
      for (int k = j; k < K; k += kGroup) {
        float w[kCols], av[kRows];
#pragma unroll
        for (int c = 0; c < kCols; ++c) w[c] = wrow[c][k];
#pragma unroll
        for (int r = 0; r < kRows; ++r) av[r] = in[r * ld + k];
#pragma unroll
        for (int r = 0; r < kRows; ++r)
#pragma unroll
          for (int c = 0; c < kCols; ++c) acc[r][c] = fmaf(av[r], w[c], acc[r][c]);
      }
    }
    // lane j of the group keeps (row j / kCols, column j % kCols)
    float mine = 0.f;
#pragma unroll
    for (int r = 0; r < kRows; ++r)
#pragma unroll
      for (int c = 0; c < kCols; ++c) {
        const float s = group_sum16(acc[r][c]);
        if (j == r * kCols + c) mine = s;
      }
    const int r = j / kCols, n = nb + j % kCols;
    if (n < N) {
      const float v = act_fwd(mine + b[n], act);
      out[r * ld + n] = v;
      if (row0 + r < B) A[(size_t)(row0 + r) * N + n] = v;
    }
  }
}

__global__ __launch_bounds__(kThreads) void k_head_fwd(const HeadArgs h) {
  extern __shared__ float4 smem4[];
  float* buf0 = reinterpret_cast<float*>(smem4);
  float* buf1 = buf0 + kRows * h.ld;
  __shared__ int s_last;
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int ld = h.ld;

  for (int i = threadIdx.x; i < kRows * h.dims[0]; i += kThreads) {
    const int r = i / h.dims[0], k = i % h.dims[0];
    buf0[r * ld + k] = row0 + r < h.B ? h.x[(size_t)(row0 + r) * h.ldx + k] : 0.f;
  }
  __syncthreads();
  float* in = buf0;
  float* out = buf1;
  for (int l = 0; l < h.L; ++l) {
    const int K = h.dims[l], N = h.dims[l + 1];
    const float* W = h.W[l];
    if (K % 4 == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0)
      layer_fwd<true>(W, h.b[l], in, out, h.a[l], K, N, h.act[l], ld, row0, h.B);
    else
      layer_fwd<false>(W, h.b[l], in, out, h.a[l], K, N, h.act[l], ld, row0, h.B);
    __syncthreads();
    float* t = in;
    in = out;
    out = t;
  }
  if (h.loss == MOLCLR_LOSS_NONE) return;

  // per-row loss (not yet divided), one thread per row, ascending columns
  const int C = h.dims[h.L];
  if (threadIdx.x < kRows && row0 + threadIdx.x < h.B) {
    const int64_t row = row0 + threadIdx.x;
    const float* p = in + threadIdx.x * ld;
    float v;
    if (h.loss == MOLCLR_LOSS_CROSS_ENTROPY) {
      const int64_t y = static_cast<const int64_t*>(h.target)[row];
      if (y < 0 || y >= C) {  // never an index
        if (h.status) atomicOr(h.status, MOLCLR_STATUS_LABEL_RANGE);
        v = __builtin_nanf("");
      } else {
        float m = p[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, p[c]);
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += expf(p[c] - m);
        v = (m + logf(s)) - p[(int)y];
      }
    } else {
      const float* t = static_cast<const float*>(h.target) + (size_t)row * C;
      v = 0.f;
      for (int c = 0; c < C; ++c) {
        const float d = p[c] - t[c];
        v = h.loss == MOLCLR_LOSS_MSE ? fmaf(d, d, v) : v + fabsf(d);
      }
    }
    h.rowloss[row] = v;
  }
  // the last workgroup to arrive reduces every row in a fixed order
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) s_last = atomicAdd(h.sync, 1) == (int)gridDim.x - 1;
  __syncthreads();
  if (!s_last || threadIdx.x >= 64) return;
  __threadfence();
  float s = 0.f;
  for (int64_t i = threadIdx.x; i < h.B; i += 64) s += agent_load(h.rowloss + i);
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) {
    const float cnt = h.loss == MOLCLR_LOSS_CROSS_ENTROPY ? (float)h.B : (float)h.B * (float)C;
    *h.loss_out = s / cnt;
    *h.sync = 0;  // ready for the next call
  }
}

__global__ __launch_bounds__(kThreads) void k_head_bwd_delta(const HeadArgs h, const GradArgs g) {
  extern __shared__ float4 smem4[];
  float* buf0 = reinterpret_cast<float*>(smem4);
  float* buf1 = buf0 + kRows * h.ld;
  __shared__ float s_max[kRows], s_sum[kRows];
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int ld = h.ld, L = h.L;
  const int C = h.dims[L];
  const float* pred = h.a[L - 1];
  const bool with_loss = h.loss != MOLCLR_LOSS_NONE && g.gloss != nullptr;

  if (with_loss && h.loss == MOLCLR_LOSS_CROSS_ENTROPY && threadIdx.x < kRows &&
      row0 + threadIdx.x < h.B) {
    const float* p = pred + (size_t)(row0 + threadIdx.x) * C;
    float m = p[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, p[c]);
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += expf(p[c] - m);
    s_max[threadIdx.x] = m;
    s_sum[threadIdx.x] = s;
  }
  __syncthreads();
  // delta_L = (dloss/dpred * gloss + dpred [+ dh when L == 1]) * act_L'
  float* cur = buf0;
  float* nxt = buf1;
  const float gl = with_loss ? *g.gloss : 0.f;
  for (int i = threadIdx.x; i < kRows * C; i += kThreads) {
    const int r = i / C, n = i % C;
    const int64_t row = row0 + r;
    float d = 0.f;
    if (row < h.B) {
      const float p = pred[(size_t)row * C + n];
      if (with_loss) {
        if (h.loss == MOLCLR_LOSS_CROSS_ENTROPY) {
          const int64_t y = static_cast<const int64_t*>(h.target)[row];
          if (y < 0 || y >= C)
            d = __builtin_nanf("");
          else
            d = gl * ((expf(p - s_max[r]) / s_sum[r] - (n == (int)y ? 1.f : 0.f)) / (float)h.B);
        } else {
          const float diff = p - static_cast<const float*>(h.target)[(size_t)row * C + n];
          const float cnt = (float)h.B * (float)C;
          if (h.loss == MOLCLR_LOSS_MSE)
            d = gl * (2.f * diff / cnt);
          else
            d = gl * ((diff > 0.f ? 1.f : diff < 0.f ? -1.f : 0.f) / cnt);
        }
      }
      if (g.dpred) d += g.dpred[(size_t)row * C + n];
      if (L == 1 && g.dh) d += g.dh[(size_t)row * C + n];
      d *= act_bwd(p, h.act[L - 1]);
      g.delta[L - 1][(size_t)row * C + n] = d;
    }
    cur[r * ld + n] = d;
  }
  __syncthreads();

  for (int l = L - 1; l >= 0; --l) {
    const int K = h.dims[l], N = h.dims[l + 1];
    if (l == 0 && !g.dx) break;
    const float* W = h.W[l];
    for (int k = threadIdx.x; k < K; k += kThreads) {
      float acc[kRows];
#pragma unroll
      for (int r = 0; r < kRows; ++r) acc[r] = 0.f;
      int n = 0;
      for (; n + 4 <= N; n += 4) {  // ld % 4 == 0: aligned float4 broadcasts
        float w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) w[q] = W[(size_t)(n + q) * K + k];
#pragma unroll
        for (int r = 0; r < kRows; ++r) {
          const float4 dv = *reinterpret_cast<const float4*>(cur + r * ld + n);
          float s = acc[r];
          s = fmaf(dv.x, w[0], s);
          s = fmaf(dv.y, w[1], s);
          s = fmaf(dv.z, w[2], s);
          s = fmaf(dv.w, w[3], s);
          acc[r] = s;
        }
      }
      for (; n < N; ++n) {
        const float w = W[(size_t)n * K + k];
#pragma unroll
        for (int r = 0; r < kRows; ++r) acc[r] = fmaf(cur[r * ld + n], w, acc[r]);
      }
#pragma unroll
      for (int r = 0; r < kRows; ++r) {
        const int64_t row = row0 + r;
        float d = acc[r];
        if (l == 0) {
          if (row < h.B) g.dx[(size_t)row * g.lddx + k] = d;
          continue;
        }
        if (row < h.B) {
          if (l == 1 && g.dh) d += g.dh[(size_t)row * K + k];
          d *= act_bwd(h.a[l - 1][(size_t)row * K + k], h.act[l - 1]);
          g.delta[l - 1][(size_t)row * K + k] = d;
        } else {
          d = 0.f;
        }
        nxt[r * ld + k] = d;
      }
    }
    __syncthreads();
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
}

// dW_l[n][k] (+)= sum_r delta_l[r][n] a_{l-1}[r][k], db_l[n] (+)= sum_r delta_l[r][n]
__global__ __launch_bounds__(kWgK) void k_head_bwd_wgrad(const HeadArgs h, const GradArgs g) {
  int l = 0;
  while (l + 1 < h.L && (int)blockIdx.x >= g.tile0[l + 1]) ++l;
  const int K = h.dims[l], N = h.dims[l + 1];
  const int kt = (K + kWgK - 1) / kWgK;
  const int tile = blockIdx.x - g.tile0[l];
  const int n0 = (tile / kt) * kWgN, k = (tile % kt) * kWgK + threadIdx.x;
  const float* A = l == 0 ? h.x : h.a[l - 1];
  const int64_t lda = l == 0 ? h.ldx : K;
  const float* D = g.delta[l];
  int nn[kWgN];
#pragma unroll
  for (int q = 0; q < kWgN; ++q) nn[q] = min(n0 + q, N - 1);

  if (g.dW[l] && k < K) {
    float acc[kWgN];
#pragma unroll
    for (int q = 0; q < kWgN; ++q) acc[q] = 0.f;
    for (int64_t r = 0; r < h.B; ++r) {
      const float av = A[(size_t)r * lda + k];
      const float* dr = D + (size_t)r * N;
#pragma unroll
      for (int q = 0; q < kWgN; ++q) acc[q] = fmaf(dr[nn[q]], av, acc[q]);
    }
#pragma unroll
    for (int q = 0; q < kWgN; ++q)
      if (n0 + q < N) {
        float* o = g.dW[l] + (size_t)(n0 + q) * K + k;
        *o = g.acc[l] ? *o + acc[q] : acc[q];
      }
  }
  if (g.db[l] && tile % kt == 0 && threadIdx.x < kWgN && n0 + (int)threadIdx.x < N) {
    const int n = n0 + threadIdx.x;
    float s = 0.f;
    for (int64_t r = 0; r < h.B; ++r) s += D[(size_t)r * N + n];
    float* o = g.db[l] + n;
    *o = g.acc[l] ? *o + s : s;
  }
}

int fill_args(const molclr_task_head* head, HeadArgs& a, const char* who) {
  MOLCLR_REQUIRE(head, "%s: null descriptor", who);
  MOLCLR_REQUIRE(head->num_layers >= 1 && head->num_layers <= kMaxL, "%s: %d layers (1..%d)", who,
                 head->num_layers, kMaxL);
  MOLCLR_REQUIRE(head->rows >= 1, "%s: rows %lld must be >= 1", who, (long long)head->rows);
  MOLCLR_REQUIRE(head->loss >= MOLCLR_LOSS_NONE && head->loss <= MOLCLR_LOSS_L1,
                 "%s: unknown loss %d", who, head->loss);
  a.L = head->num_layers;
  a.loss = head->loss;
  a.B = head->rows;
  int dmax = 0;
  for (int l = 0; l <= a.L; ++l) {
    MOLCLR_REQUIRE(head->dims[l] >= 1, "%s: width %lld of layer %d must be >= 1", who,
                   (long long)head->dims[l], l);
    if (head->dims[l] > kMaxDim) {
      molclr::set_error("%s: width %lld of layer %d exceeds %d (the row block's LDS buffers)",
                        who, (long long)head->dims[l], l, kMaxDim);
      return MOLCLR_ERR_UNSUPPORTED;
    }
    a.dims[l] = (int)head->dims[l];
    dmax = a.dims[l] > dmax ? a.dims[l] : dmax;
  }
  MOLCLR_REQUIRE(head->rows * (int64_t)dmax < ((int64_t)1 << 40), "%s: rows too large", who);
  a.ld = (dmax + 3) / 4 * 4;
  for (int l = 0; l < a.L; ++l) {
    MOLCLR_REQUIRE(head->act[l] >= MOLCLR_ACT_NONE && head->act[l] <= MOLCLR_ACT_SOFTPLUS,
                   "%s: unknown activation %d of layer %d", who, head->act[l], l);
    MOLCLR_REQUIRE(head->weight[l] && head->bias[l] && head->a[l],
                   "%s: null weight / bias / activation pointer of layer %d", who, l);
    a.act[l] = head->act[l];
    a.W[l] = head->weight[l];
    a.b[l] = head->bias[l];
    a.a[l] = head->a[l];
  }
  MOLCLR_REQUIRE(head->x && head->ldx >= head->dims[0], "%s: x is null or ldx < dims[0]", who);
  a.x = head->x;
  a.ldx = head->ldx;
  if (a.loss != MOLCLR_LOSS_NONE) {
    MOLCLR_REQUIRE(head->target, "%s: the loss needs a target", who);
    MOLCLR_REQUIRE(a.loss != MOLCLR_LOSS_CROSS_ENTROPY || a.dims[a.L] <= MOLCLR_TASK_HEAD_MAX_CLASSES,
                   "%s: cross-entropy over %d classes (at most %d)", who, a.dims[a.L],
                   MOLCLR_TASK_HEAD_MAX_CLASSES);
  }
  a.target = head->target;
  a.loss_out = head->loss_out;
  a.status = head->status;
  a.sync = head->sync;
  a.rowloss = nullptr;
  return MOLCLR_OK;
}

size_t delta_floats(const molclr_task_head* head) {
  size_t n = 0;
  for (int l = 0; l < head->num_layers; ++l)
    n += molclr::align_up((size_t)head->rows * (size_t)head->dims[l + 1], 64);
  return n;
}

}  // namespace

MOLCLR_API size_t molclr_task_head_workspace_bytes(const molclr_task_head* head) {
  if (!head || head->num_layers < 1 || head->num_layers > kMaxL || head->rows < 1) return 0;
  for (int l = 0; l <= head->num_layers; ++l)
    if (head->dims[l] < 1 || head->dims[l] > kMaxDim) return 0;
  return 256 * (size_t)(head->num_layers + 2) + sizeof(float) * ((size_t)head->rows + delta_floats(head));
}

MOLCLR_API int molclr_task_head_fwd(const molclr_task_head* head, void* workspace,
                                    size_t workspace_bytes, molclr_stream_t stream) {
  HeadArgs a;
  MOLCLR_TRY_RC(fill_args(head, a, "task_head_fwd"));
  if (a.loss != MOLCLR_LOSS_NONE) {
    MOLCLR_REQUIRE(a.loss_out && a.sync, "task_head_fwd: the loss needs loss_out and sync");
    MOLCLR_REQUIRE_WS(workspace_bytes, sizeof(float) * (size_t)a.B);
    MOLCLR_REQUIRE(workspace, "task_head_fwd: null workspace");
    a.rowloss = static_cast<float*>(workspace);
  }
  const int64_t blocks = molclr::ceil_div(a.B, kRows);
  MOLCLR_REQUIRE(blocks < ((int64_t)1 << 31), "task_head_fwd: rows too large");
  hipLaunchKernelGGL(k_head_fwd, dim3((unsigned)blocks), dim3(kThreads),
                     2 * kRows * a.ld * sizeof(float), molclr::as_stream(stream), a);
  MOLCLR_LAUNCHED();
  return MOLCLR_OK;
}

MOLCLR_API int molclr_task_head_bwd(const molclr_task_head* head,
                                    const molclr_task_head_grads* grads, void* workspace,
                                    size_t workspace_bytes, molclr_stream_t stream) {
  HeadArgs a;
  MOLCLR_TRY_RC(fill_args(head, a, "task_head_bwd"));
  MOLCLR_REQUIRE(grads, "task_head_bwd: null gradient descriptor");
  MOLCLR_REQUIRE(!grads->dx || grads->lddx >= a.dims[0], "task_head_bwd: lddx < dims[0]");
  MOLCLR_REQUIRE_WS(workspace_bytes, molclr_task_head_workspace_bytes(head));
  MOLCLR_REQUIRE(workspace, "task_head_bwd: null workspace");
  GradArgs g;
  g.gloss = grads->gloss;
  g.dh = grads->dh;
  g.dpred = grads->dpred;
  g.dx = grads->dx;
  g.lddx = grads->lddx;
  molclr::Workspace ws(workspace, workspace_bytes);
  int tiles = 0;
  for (int l = 0; l < a.L; ++l) {
    g.delta[l] = ws.take<float>((size_t)a.B * a.dims[l + 1]);
    g.dW[l] = grads->dweight[l];
    g.db[l] = grads->dbias[l];
    g.acc[l] = grads->accumulate[l];
    g.tile0[l] = tiles;
    if (g.dW[l] || g.db[l])
      tiles += (int)(molclr::ceil_div(a.dims[l + 1], kWgN) * molclr::ceil_div(a.dims[l], kWgK));
  }
  g.tile0[a.L] = tiles;
  if (!ws.ok()) {
    molclr::set_error("task_head_bwd: workspace too small");
    return MOLCLR_ERR_WORKSPACE;
  }
  hipStream_t s = molclr::as_stream(stream);
  hipLaunchKernelGGL(k_head_bwd_delta, dim3((unsigned)molclr::ceil_div(a.B, kRows)),
                     dim3(kThreads), 2 * kRows * a.ld * sizeof(float), s, a, g);
  MOLCLR_LAUNCHED();
  if (tiles > 0) {
    hipLaunchKernelGGL(k_head_bwd_wgrad, dim3((unsigned)tiles), dim3(kWgK), 0, s, a, g);
    MOLCLR_LAUNCHED();
  }
  return MOLCLR_OK;
}
