// GIN encoder executor: GINet's node-embedding stack (models/ginet_molclr.py:98-111)
// forward and backward as single calls over the library's own entry points.
//
// The per-op autograd path (molclr_amd/ops.py) pays ~30 us of Python per
// operation — ~4 ms of host time per training step, against ~6 ms of GPU
// time.  This file issues the same entry points, with the same arguments and
// in the same order, from C++: the kernels and their results are identical,
// only the host cost goes.
//
// Arena (saved for the backward), per layer l: agg_l [N,D], a1_l [N,2D],
// z_l [N,D], mean_l / invstd_l [D] and the BatchNorm apply coefficients
// coef_l [2][segments][D]; then h0 [N,D] (atom embedding) and the combined
// edge tables Ec [L,15,D].  The BatchNorm output h_l of every layer but the
// last is never stored: layer l + 1's aggregation applies coef_l to z_l as it
// gathers (molclr_gine_aggregate_bn_fwd; the backward reads z, never h).  The
// last layer's apply writes h_out.  MOLCLR_AGG_BN=0 (an A/B switch) keeps the
// stored h_l [N,D] and the plain gather.
// Dropout (training, drop_ratio > 0) follows every BatchNorm (+ReLU) as a
// counter-based mask (dropout.h) recomputed wherever h_l is: in the apply that
// stores it, in the next layer's gather, in the BatchNorm backward.  The
// forward's first launch copies (seed, call counter) from drop_state into the
// arena's dropkey slot and advances the counter; every kernel of the call,
// and of its backward, reads the key from the arena.
// Workspace: backward scratch dh, dz, dagg [N,D] + dz1 [N,2D], then the
// largest workspace any called entry point asks for.
#include "common.h"

#include <stdlib.h>

namespace {

// the next layer's aggregation applies the BatchNorm (default) or reads a
// stored h_l (MOLCLR_AGG_BN=0)
bool agg_bn() {
  static const bool on = !molclr::env_is("MOLCLR_AGG_BN", '0');
  return on;
}

// byte offsets; node-feature buffers in the encoder's storage type (fp32 or
// bf16), statistics and edge tables fp32; every buffer 256-byte aligned
struct ArenaLayout {
  size_t agg[MOLCLR_MAX_LAYERS], a1[MOLCLR_MAX_LAYERS], z[MOLCLR_MAX_LAYERS],
      h[MOLCLR_MAX_LAYERS], mean[MOLCLR_MAX_LAYERS], invstd[MOLCLR_MAX_LAYERS],
      coef[MOLCLR_MAX_LAYERS];
  size_t bits[MOLCLR_MAX_LAYERS];  // h3: ReLU mask of a1_l as bits [ceil(2D / 32)][N]
  size_t h0, ec, smax, bmax, dropkey, total;
  ArenaLayout(int L, int64_t N, int64_t D, size_t es) {
    size_t used = 0;
    auto off = [&](size_t bytes) {
      const size_t o = used;
      used += (bytes + 255) / 256 * 256;
      return o;
    };
    for (int l = 0; l < L; ++l) {
      agg[l] = off(N * D * es);
      a1[l] = off(N * 2 * D * es);
      z[l] = off(N * D * es);
      h[l] = agg_bn() ? 0 : off(N * D * es);  // stored only on the MOLCLR_AGG_BN=0 path
      mean[l] = off(MOLCLR_MAX_SEGMENTS * D * sizeof(float));  // [segment][D]
      invstd[l] = off(MOLCLR_MAX_SEGMENTS * D * sizeof(float));
      coef[l] = off(2 * MOLCLR_MAX_SEGMENTS * D * sizeof(float));  // scale, shift [segment][D]
      bits[l] = off((size_t)N * ((2 * D + 31) / 32) * sizeof(uint32_t));
    }
    h0 = off(N * D * es);
    ec = off((size_t)L * MOLCLR_NUM_ECOMB * D * sizeof(float));
    smax = off((size_t)MOLCLR_MAX_LAYERS * 2 * kMaxSlotFloats * sizeof(float));  // h3: max |agg_l|, |a1_l|
    // h3: the backward's max |dz_l|, |dz1_l| (zeroed by the forward with smax)
    bmax = off((size_t)MOLCLR_MAX_LAYERS * 2 * kMaxSlotFloats * sizeof(float));
    dropkey = off(2 * sizeof(int64_t));  // this forward's dropout key (seed, call)
    total = used;
  }
};

size_t elem_bytes(int dtype) { return dtype == MOLCLR_DTYPE_BF16 ? 2 : 4; }

size_t kernels_ws(int64_t N, int64_t D) {
  size_t m = 0;
  auto mx = [&](size_t v) { m = v > m ? v : m; };
  mx(molclr_gemm_f32_workspace_bytes(2 * D, D, N));  // dW0 = dz1^T agg
  mx(molclr_gemm_f32_workspace_bytes(D, 2 * D, N));  // dW2 = dz^T a1
  mx(molclr_gemm_f32_workspace_bytes(N, 2 * D, D));
  mx(molclr_gemm_f32_workspace_bytes(N, D, 2 * D));
  mx(molclr_colsum_f32_workspace_bytes(N, 2 * D));
  mx(molclr_linear_wgrad_workspace_bytes(N, D, 2 * D));
  mx(molclr_linear_wgrad_workspace_bytes(N, 2 * D, D));
  if (N >= 1024 && D % 4 == 0) mx(molclr_linear_wgrad_h3_pair_workspace_bytes(N, D, 2 * D, 2 * D, D));
  mx(molclr_linear_wgrad_bf16_workspace_bytes(N, D, 2 * D));
  mx(molclr_linear_wgrad_bf16_workspace_bytes(N, 2 * D, D));
  mx(molclr_batchnorm_ws_bound(N, D));
  mx(molclr_gine_aggregate_bwd_workspace_bytes(N, D));
  mx(molclr_atom_embed_bwd_workspace_bytes(N, D, MOLCLR_NUM_ATOM_TYPE, MOLCLR_NUM_CHIRALITY));
  return m;
}

// backward scratch dh, dz, dagg [N,D] + dz1 [N,2D], in the storage type
size_t scratch_bytes(int64_t N, int64_t D, size_t es) { return ((size_t)N * D * 3 + (size_t)N * 2 * D) * es; }

// The `training` field of either encoder struct (MOLCLR_MODE_*): the
// BatchNorms take batch statistics in MOLCLR_MODE_TRAIN alone, the dropout is
// drawn in every mode but MOLCLR_MODE_EVAL.
template <typename E>
int bn_batch_stats(const E* e) { return e->training == MOLCLR_MODE_TRAIN; }

// the mode and dropout fields of either encoder struct
int check_drop(const char* who, double drop_ratio, const int64_t* drop_state, int training) {
  MOLCLR_REQUIRE(training == MOLCLR_MODE_EVAL || training == MOLCLR_MODE_TRAIN ||
                     training == MOLCLR_MODE_FROZEN_BN,
                 "%s: training %d (MOLCLR_MODE_*)", who, training);
  MOLCLR_REQUIRE(drop_ratio >= 0.0 && drop_ratio < 1.0, "%s: drop_ratio %g outside [0, 1)", who,
                 drop_ratio);
  MOLCLR_REQUIRE(!(training && drop_ratio > 0.0) || drop_state,
                 "%s: training with dropout needs drop_state", who);
  return MOLCLR_OK;
}

int check_encoder(const molclr_gin_encoder* e, const molclr_device_graph* g) {
  MOLCLR_REQUIRE(e && g, "gin_encoder: null encoder / graph");
  MOLCLR_TRY_RC(check_drop("gin_encoder", e->drop_ratio, e->drop_state, e->training));
  MOLCLR_REQUIRE(e->num_layer >= 1 && e->num_layer <= MOLCLR_MAX_LAYERS,
                 "gin_encoder: num_layer %d", e->num_layer);
  MOLCLR_REQUIRE(e->dim > 0 && e->dim % 4 == 0, "gin_encoder: dim %lld", (long long)e->dim);
  MOLCLR_REQUIRE(e->dtype == MOLCLR_DTYPE_F32 || (e->dtype == MOLCLR_DTYPE_BF16 && e->dim % 8 == 0),
                 "gin_encoder: dtype %d (bf16 needs dim %% 8 == 0)", e->dtype);
  MOLCLR_REQUIRE(e->n_atom == MOLCLR_NUM_ATOM_TYPE && e->n_chiral == MOLCLR_NUM_CHIRALITY,
                 "gin_encoder: embedding tables must be [%d,D] and [%d,D]",
                 MOLCLR_NUM_ATOM_TYPE, MOLCLR_NUM_CHIRALITY);
  for (int l = 0; l < e->num_layer; ++l)
    MOLCLR_REQUIRE(e->mlp0_planes[l] && e->mlp0_planes_t[l] && e->mlp2_planes[l] &&
                       e->mlp2_planes_t[l] && e->bn_weight[l] && e->bn_bias[l],
                   "gin_encoder: layer %d: missing planes or BatchNorm affine", l);
  return MOLCLR_OK;
}

// BatchNorm segments of a graph (the views of a paired forward), checked
// (device-sized graph: the rows of every segment are read on the device,
// g->num_nodes rows in all, the rest padding)
struct SegRows {
  int n;
  const int64_t* rows;
  const int64_t* dev;
  int64_t cap;
};
int graph_segments(const molclr_device_graph* g, const int64_t* N, SegRows& out) {
  if (g->segment_nodes_dev) {
    MOLCLR_REQUIRE(g->num_segments >= 1 && g->num_segments <= MOLCLR_MAX_SEGMENTS,
                   "encoder: %d graph segments", g->num_segments);
    out = {g->num_segments, nullptr, g->segment_nodes_dev, *N};
    return MOLCLR_OK;
  }
  if (g->num_segments <= 1) {
    out = {1, N, nullptr, *N};
    return MOLCLR_OK;
  }
  MOLCLR_REQUIRE(g->num_segments <= MOLCLR_MAX_SEGMENTS, "encoder: %d graph segments",
                 g->num_segments);
  int64_t tot = 0;
  for (int s = 0; s < g->num_segments; ++s) tot += g->segment_nodes[s];
  MOLCLR_REQUIRE(tot == *N, "encoder: segment nodes sum to %lld, graph has %lld", (long long)tot,
                 (long long)*N);
  out = {g->num_segments, g->segment_nodes, nullptr, *N};
  return MOLCLR_OK;
}

// the segmented BatchNorm of a graph, host- or device-sized (molclr::bn_forward
// / bn_backward); drop: the dropout after it (NULL: none).  `who`: the entry
// point of norm.hip that makes the same call, which a refusal names.
molclr::BnSegs bn_segs(const SegRows& sg, const char* who, int64_t D, int dtype,
                       const DropArgs* drop, void* ws, size_t ws_bytes, molclr_stream_t stream) {
  return {who, sg.n, sg.rows, sg.dev, sg.cap, D, dtype, ws, ws_bytes, molclr::as_stream(stream),
          drop};
}
int seg_bn_fwd(const SegRows& sg, const void* z, const float* gamma, const float* beta,
               float* rmean, float* rvar, int64_t* nbt, void* y, float* mean, float* invstd,
               int64_t D, int dtype, double momentum, double eps, int training, int relu,
               const DropArgs* drop, void* ws, size_t ws_bytes, molclr_stream_t stream) {
  const char* who = drop     ? "batchnorm_seg_fwd_drop"
                    : sg.dev ? "batchnorm_seg_fwd_dev"
                             : "batchnorm_seg_fwd";
  return molclr::bn_forward({bn_segs(sg, who, D, dtype, drop, ws, ws_bytes, stream), z, gamma,
                             beta, rmean, rvar, nbt, y, mean, invstd, nullptr, momentum, eps,
                             training, relu});
}
// its statistics and apply coefficients only (coef: scale, shift [sg.n][D])
int seg_bn_coeffs(const SegRows& sg, const void* z, const float* gamma, const float* beta,
                  float* rmean, float* rvar, int64_t* nbt, float* mean, float* invstd, float* coef,
                  int64_t D, int dtype, double momentum, double eps, int training, void* ws,
                  size_t ws_bytes, molclr_stream_t stream) {
  const char* who = sg.dev ? "batchnorm_seg_coeffs_dev" : "batchnorm_seg_coeffs";
  return molclr::bn_forward({bn_segs(sg, who, D, dtype, nullptr, ws, ws_bytes, stream), z, gamma,
                             beta, rmean, rvar, nbt, nullptr, mean, invstd, coef, momentum, eps,
                             training, 0});
}
// rowmax != NULL (fp32): also dz's row maxima and max slot (the h3 scales)
// frozen: mean / invstd are the running statistics an eval-mode forward saved
int seg_bn_bwd(const SegRows& sg, int frozen, const void* dy, const void* z, const float* gamma,
               const float* beta, const float* mean, const float* invstd, void* dz, float* dgamma,
               float* dbeta, int64_t D, int dtype, int relu, int accumulate, float* rowmax,
               float* slot, const DropArgs* drop, void* ws, size_t ws_bytes,
               molclr_stream_t stream) {
  const char* who = frozen   ? "batchnorm_seg_bwd_frozen"
                    : drop   ? "batchnorm_seg_bwd_drop"
                    : sg.dev ? "batchnorm_seg_bwd_dev"
                    : rowmax ? "batchnorm_seg_bwd_max"
                             : "batchnorm_seg_bwd";
  return molclr::bn_backward({bn_segs(sg, who, D, dtype, drop, ws, ws_bytes, stream), dy, z, gamma,
                              beta, mean, invstd, dz, dgamma, dbeta, relu, accumulate, rowmax,
                              slot, frozen});
}

// This call's dropout: the key in the arena, opened by the forward
// (open_drop); at(l): the arguments of the dropout after layer l's BatchNorm,
// NULL when the call has none.
struct CallDrop {
  bool on;
  double p;
  const int64_t* key;
  DropArgs cur;
  CallDrop(int training, double drop_ratio, const void* key_slot)
      : on(training && drop_ratio > 0.0), p(drop_ratio), key((const int64_t*)key_slot), cur{} {}
  const DropArgs* at(int l) {
    if (!on) return nullptr;
    cur = make_drop_args(key, p, l);
    return &cur;
  }
};
int open_drop(const CallDrop& d, int64_t* state, molclr_stream_t stream) {
  if (!d.on) return MOLCLR_OK;
  return molclr_dropout_next_key(state, const_cast<int64_t*>(d.key), stream);
}

#define MOLCLR_TRY(expr)      \
  do {                        \
    int rc_ = (expr);         \
    if (rc_) return rc_;      \
  } while (0)

// the grads struct's optional "gradients final" events (layer_done / embed_done)
int record_done(void* ev, molclr_stream_t stream) {
  if (ev && hipEventRecord(static_cast<hipEvent_t>(ev), molclr::as_stream(stream)) != hipSuccess) {
    molclr::set_error("encoder_bwd: hipEventRecord failed");
    return MOLCLR_ERR_ARG;
  }
  return MOLCLR_OK;
}

}  // namespace

MOLCLR_API size_t molclr_gin_encoder_arena_bytes(int L, int64_t N, int64_t D, int dtype) {
  if (L < 1 || L > MOLCLR_MAX_LAYERS) return 0;
  return ArenaLayout(L, N, D, elem_bytes(dtype)).total;
}

// workspace: backward scratch | h3 max slots of dz_l / dz1_l | h3 row maxima
// of agg / dz [N] and of a1 / dz1 [parts][N] | the entry points' workspace
constexpr size_t kSlotBytes = MOLCLR_MAX_LAYERS * 2 * kMaxSlotFloats * sizeof(float);
// row maxima of a [N,D] tensor and of a [N,2D] GEMM output
// (molclr_gemm_row_parts(2D) partial arrays)
// the first region: dz's row-max parts, or agg's in the aggregation's layout
// (h3 forward, molclr_rowmax_layout)
size_t rowmax_first_bytes(int64_t N, int64_t D) {
  const size_t dz = (size_t)molclr_bn_row_parts(D) * N * sizeof(float);
  const size_t agg = molclr_rowmax_bytes(N, D);
  return molclr::align_up(dz > agg ? dz : agg, 256);
}
size_t rowmax_bytes(int64_t N, int64_t D) {
  return molclr::align_up(
      rowmax_first_bytes(N, D) + (size_t)molclr_gemm_row_parts(2 * D) * N * sizeof(float), 256);
}

MOLCLR_API size_t molclr_gin_encoder_workspace_bytes(int L, int64_t N, int64_t D, int dtype) {
  (void)L;
  return molclr::align_up(scratch_bytes(N, D, elem_bytes(dtype)), 256) + kSlotBytes +
         rowmax_bytes(N, D) + kernels_ws(N, D) + 256;
}

MOLCLR_API int molclr_gin_encoder_fwd(const molclr_gin_encoder* e, const int64_t* x,
                                      const molclr_device_graph* g, void* h_out, void* arena,
                                      size_t arena_bytes, void* workspace, size_t workspace_bytes,
                                      molclr_stream_t stream) {
  MOLCLR_TRY(check_encoder(e, g));
  const int L = e->num_layer;
  const int64_t N = g->num_nodes, D = e->dim;
  if (N == 0) return MOLCLR_OK;
  SegRows seg;
  MOLCLR_TRY(graph_segments(g, &g->num_nodes, seg));
  MOLCLR_REQUIRE(x && h_out && arena, "gin_encoder_fwd: null pointer");
  const bool bf = e->dtype == MOLCLR_DTYPE_BF16;
  const size_t es = elem_bytes(e->dtype);
  const ArenaLayout lay(L, N, D, es);
  MOLCLR_REQUIRE_WS(arena_bytes, lay.total);
  MOLCLR_REQUIRE_WS(workspace_bytes, molclr_gin_encoder_workspace_bytes(L, N, D, e->dtype));
  char* A = (char*)arena;
  auto F = [&](size_t off) { return (float*)(A + off); };
  auto H = [&](size_t off) { return (uint16_t*)(A + off); };
  // h3: row maxima of agg and a1 (workspace row-maxima region)
  float* ragg = (float*)((char*)workspace + molclr::align_up(scratch_bytes(N, D, es), 256) +
                         kSlotBytes);
  float* ra1 = (float*)((char*)ragg + rowmax_first_bytes(N, D));  // after agg's row maxima
  void* kws = (char*)ragg + rowmax_bytes(N, D);
  const size_t kws_bytes = kernels_ws(N, D);
  const bool h3 = !bf && e->fp32_gemm != 0;
  const bool h3f = h3 && (e->fp32_gemm & 2);  // h3 forward products (not the default)
  float* fmax = F(lay.smax);  // h3: [l][0] = max |agg_l|, [l][1] = max |a1_l|

  // layer l > 0 gathers from z_{l-1} through coef_{l-1} (fused), else from h
  const bool fused = agg_bn();
  CallDrop drop(e->training, e->drop_ratio, A + lay.dropkey);
  MOLCLR_TRY(open_drop(drop, e->drop_state, stream));
  void* h = A + lay.h0;
  if (bf)
    MOLCLR_TRY(molclr_atom_embed_fwd_bf16(x, e->x_embedding1, e->x_embedding2, (uint16_t*)h, N, D,
                                          e->n_atom, e->n_chiral, e->status, stream));
  else
    MOLCLR_TRY(molclr_atom_embed_fwd(x, e->x_embedding1, e->x_embedding2, (float*)h, N, D,
                                     e->n_atom, e->n_chiral, e->status, stream));
  float* Ec = F(lay.ec);
  // h3: the forward's and the backward's max slots (smax, bmax: adjacent)
  // zeroed by the same launch
  const int64_t nz = h3 ? (int64_t)(lay.bmax - lay.smax) / 4 + (int64_t)L * 2 * kMaxSlotFloats : 0;
  MOLCLR_TRY(molclr::edge_tables_combine_zero(L, e->edge_embedding1, e->edge_embedding2, Ec, D,
                                              h3 ? fmax : nullptr, nz, stream));
  for (int l = 0; l < L; ++l) {
    const bool last = l == L - 1;
    const bool bn_src = fused && l > 0;   // this layer's source: z_{l-1} with coef_{l-1}
    const bool bn_next = fused && !last;  // this layer's BatchNorm: coefficients only
    void* y = last ? h_out : bn_next ? nullptr : A + lay.h[l];
    const float* Ecl = Ec + (size_t)l * MOLCLR_NUM_ECOMB * D;
    const void* zp = bn_src ? A + lay.z[l - 1] : nullptr;
    const float* cp = bn_src ? F(lay.coef[l - 1]) : nullptr;
    if (bf) {
      uint16_t *agg = H(lay.agg[l]), *a1 = H(lay.a1[l]), *z = H(lay.z[l]);
      if (bn_src && drop.on)
        MOLCLR_TRY(molclr::gine_aggregate_bn_fwd_drop(zp, cp, 1, seg.n, seg.rows, seg.dev,
                                                      g->rowptr, g->col, g->ecode, g->nbr, Ecl,
                                                      agg, N, D, MOLCLR_DTYPE_BF16, nullptr,
                                                      nullptr, *drop.at(l - 1),
                                                      molclr::as_stream(stream)));
      else if (bn_src)
        MOLCLR_TRY(molclr_gine_aggregate_bn_fwd_bf16((const uint16_t*)zp, cp, 1, seg.n, seg.rows,
                                                     seg.dev, g->rowptr, g->col, g->ecode, g->nbr,
                                                     Ecl, agg, N, D, stream));
      else
        MOLCLR_TRY(molclr_gine_aggregate_fwd_bf16((const uint16_t*)h, g->rowptr, g->col, g->ecode,
                                                  g->nbr, Ecl, agg, N, D, stream));
      // GINEConv.update in bf16: one MFMA per product, fp32 accumulation; the
      // first product also writes a1's ReLU mask as bits for the backward
      if (D % 64 == 0)
        MOLCLR_TRY(molclr_gemm_bf16_bits(agg, e->mlp0_planes[l], a1, N, 2 * D, D, D, 2 * D,
                                         MOLCLR_EPI_BIAS_RELU, e->mlp0_bias[l],
                                         (uint32_t*)(A + lay.bits[l]), nullptr, stream));
      else
        MOLCLR_TRY(molclr_gemm_bf16(agg, e->mlp0_planes[l], a1, N, 2 * D, D, D, 2 * D,
                                    MOLCLR_EPI_BIAS_RELU, e->mlp0_bias[l], nullptr, 0, stream));
      MOLCLR_TRY(molclr_gemm_bf16(a1, e->mlp2_planes[l], z, N, D, 2 * D, 2 * D, D,
                                  MOLCLR_EPI_BIAS, e->mlp2_bias[l], nullptr, 0, stream));
      if (bn_next)
        MOLCLR_TRY(seg_bn_coeffs(seg, z, e->bn_weight[l], e->bn_bias[l], e->bn_running_mean[l],
                                 e->bn_running_var[l], e->bn_num_batches_tracked[l],
                                 F(lay.mean[l]), F(lay.invstd[l]), F(lay.coef[l]), D,
                                 MOLCLR_DTYPE_BF16, e->momentum, e->eps, bn_batch_stats(e), kws,
                                 kws_bytes, stream));
      else
        MOLCLR_TRY(seg_bn_fwd(seg, z, e->bn_weight[l], e->bn_bias[l], e->bn_running_mean[l],
                              e->bn_running_var[l], e->bn_num_batches_tracked[l], y,
                              F(lay.mean[l]), F(lay.invstd[l]), D, MOLCLR_DTYPE_BF16, e->momentum,
                              e->eps, bn_batch_stats(e), last ? 0 : 1, drop.at(l), kws, kws_bytes,
                              stream));
    } else {
      float *agg = F(lay.agg[l]), *a1 = F(lay.a1[l]), *z = F(lay.z[l]);
      float* sl = fmax + 2 * l * kMaxSlotFloats;
      // h3 forward: agg's row maxima from the aggregation itself, max |agg| from lin1
      if (bn_src && drop.on)
        MOLCLR_TRY(molclr::gine_aggregate_bn_fwd_drop(zp, cp, 1, seg.n, seg.rows, seg.dev,
                                                      g->rowptr, g->col, g->ecode, g->nbr, Ecl,
                                                      agg, N, D, MOLCLR_DTYPE_F32,
                                                      h3f ? ragg : nullptr, nullptr,
                                                      *drop.at(l - 1), molclr::as_stream(stream)));
      else if (bn_src)
        MOLCLR_TRY(molclr_gine_aggregate_bn_fwd((const float*)zp, cp, 1, seg.n, seg.rows, seg.dev,
                                                g->rowptr, g->col, g->ecode, g->nbr, Ecl, agg, N,
                                                D, h3f ? ragg : nullptr, nullptr, stream));
      else if (h3f)
        MOLCLR_TRY(molclr_gine_aggregate_fwd_rowmax((const float*)h, g->rowptr, g->col, g->ecode,
                                                    g->nbr, Ecl, agg, N, D, ragg, nullptr,
                                                    stream));
      else
        MOLCLR_TRY(molclr_gine_aggregate_fwd((const float*)h, g->rowptr, g->col, g->ecode, g->nbr,
                                             Ecl, agg, N, D, stream));
      if (h3f) {
        // GINEConv.update in h3 (ops._MLP), A scaled row by row; max |agg| (its
        // A reads), max |a1|, a1's row maxima and its ReLU mask as bits from
        // the first GEMM
        const uint16_t* p0 = e->mlp0_planes[l];
        const uint16_t* p2 = e->mlp2_planes[l];
        MOLCLR_TRY(molclr_gemm_f32_h3_bits(agg, ragg, (int)molclr_rowmax_layout(D), p0, a1, N,
                                           2 * D, D, D, 2 * D, MOLCLR_EPI_BIAS_RELU,
                                           e->mlp0_bias[l], nullptr, 0, nullptr,
                                           sl + kMaxSlotFloats, ra1, sl,
                                           (uint32_t*)(A + lay.bits[l]), stream));
        MOLCLR_TRY(molclr_gemm_f32_h3(a1, ra1, (int)molclr_gemm_row_parts(2 * D), p2, z, N, D,
                                      2 * D, 2 * D, D, MOLCLR_EPI_BIAS, e->mlp2_bias[l], nullptr, 0,
                                      nullptr,
                                      nullptr, nullptr, nullptr, stream));
      } else {
        // GINEConv.update: Linear(D,2D) + ReLU, Linear(2D,D)  (ops.linear_fwd);
        // h3 backward: the first product also yields max |agg| and max |a1|
        if (h3)
          MOLCLR_TRY(molclr_gemm_f32_bplanes_max(agg, e->mlp0_planes[l], a1, N, 2 * D, D, D, 2 * D,
                                                 MOLCLR_EPI_BIAS_RELU, e->mlp0_bias[l], nullptr, 0,
                                                 fmax + 2 * l * kMaxSlotFloats,
                                                 fmax + (2 * l + 1) * kMaxSlotFloats, nullptr,
                                                 (uint32_t*)(A + lay.bits[l]), kws, kws_bytes,
                                                 stream));
        else
          MOLCLR_TRY(molclr_gemm_f32_bplanes(agg, e->mlp0_planes[l], a1, N, 2 * D, D, D, 2 * D, 0,
                                             MOLCLR_EPI_BIAS_RELU, e->mlp0_bias[l], nullptr, 0, kws,
                                             kws_bytes, stream));
        MOLCLR_TRY(molclr_gemm_f32_bplanes(a1, e->mlp2_planes[l], z, N, D, 2 * D, 2 * D, D, 0,
                                           MOLCLR_EPI_BIAS, e->mlp2_bias[l], nullptr, 0, kws,
                                           kws_bytes, stream));
      }
      if (bn_next)
        MOLCLR_TRY(seg_bn_coeffs(seg, z, e->bn_weight[l], e->bn_bias[l], e->bn_running_mean[l],
                                 e->bn_running_var[l], e->bn_num_batches_tracked[l],
                                 F(lay.mean[l]), F(lay.invstd[l]), F(lay.coef[l]), D,
                                 MOLCLR_DTYPE_F32, e->momentum, e->eps, bn_batch_stats(e), kws, kws_bytes,
                                 stream));
      else
        MOLCLR_TRY(seg_bn_fwd(seg, z, e->bn_weight[l], e->bn_bias[l], e->bn_running_mean[l],
                              e->bn_running_var[l], e->bn_num_batches_tracked[l], y,
                              F(lay.mean[l]), F(lay.invstd[l]), D, MOLCLR_DTYPE_F32, e->momentum,
                              e->eps, bn_batch_stats(e), last ? 0 : 1, drop.at(l), kws, kws_bytes,
                              stream));
    }
    h = y;
  }
  return MOLCLR_OK;
}

MOLCLR_API int molclr_gin_encoder_bwd(const molclr_gin_encoder* e,
                                      const molclr_gin_encoder_grads* gr, const int64_t* x,
                                      const molclr_device_graph* g, const void* dh_out,
                                      const void* arena, size_t arena_bytes, void* workspace,
                                      size_t workspace_bytes, molclr_stream_t stream) {
  MOLCLR_TRY(check_encoder(e, g));
  MOLCLR_REQUIRE(gr, "gin_encoder_bwd: null grads");
  const int L = e->num_layer;
  const int64_t N = g->num_nodes, D = e->dim;
  if (N == 0) return MOLCLR_OK;
  SegRows seg;
  MOLCLR_TRY(graph_segments(g, &g->num_nodes, seg));
  MOLCLR_REQUIRE(x && dh_out && arena, "gin_encoder_bwd: null pointer");
  const bool bf = e->dtype == MOLCLR_DTYPE_BF16;
  const size_t es = elem_bytes(e->dtype);
  const ArenaLayout lay(L, N, D, es);
  MOLCLR_REQUIRE_WS(arena_bytes, lay.total);
  MOLCLR_REQUIRE_WS(workspace_bytes, molclr_gin_encoder_workspace_bytes(L, N, D, e->dtype));
  const char* A = (const char*)arena;
  auto F = [&](size_t off) { return (const float*)(A + off); };
  char* S = (char*)workspace;
  void* dh = S;                              // gradient w.r.t. the current layer's output
  void* dz = S + (size_t)N * D * es;         // w.r.t. the BatchNorm input z
  void* dagg = S + 2 * (size_t)N * D * es;   // w.r.t. the aggregation output
  void* dz1 = S + 3 * (size_t)N * D * es;    // w.r.t. the first Linear's pre-activation [N,2D]
  // h3: the arena's backward slots, zeroed by the forward (a second backward
  // of the same forward folds the same maxima again: the same values)
  float* bmax = const_cast<float*>(F(lay.bmax));
  float* rdz = (float*)(S + molclr::align_up(scratch_bytes(N, D, es), 256)) +
               kSlotBytes / sizeof(float);  // h3: row maxima of dz, then of dz1
  float* rdz1 = (float*)((char*)rdz + rowmax_first_bytes(N, D));  // after dz's row maxima
  void* kws = (char*)rdz + rowmax_bytes(N, D);
  const size_t kws_bytes = kernels_ws(N, D);
  const int dt = bf ? MOLCLR_DTYPE_BF16 : MOLCLR_DTYPE_F32;
  const bool h3 = !bf && e->fp32_gemm != 0;
  const float* fmax = F(lay.smax);  // the forward's max |agg_l|, max |a1_l|
  // h3: bmax[l][0] = max |dz_l|, [l][1] = max |dz1_l|
  CallDrop drop(e->training, e->drop_ratio, A + lay.dropkey);  // the forward's key

  const void* dy = dh_out;
  for (int l = L - 1; l >= 0; --l) {
    const void* agg = A + lay.agg[l];
    const void* a1 = A + lay.a1[l];
    const void* z = A + lay.z[l];
    const bool last = l == L - 1;
    MOLCLR_REQUIRE(gr->bn_weight[l] && gr->bn_bias[l], "gin_encoder_bwd: BatchNorm grads needed");
    if (h3) {
      // dz's row maxima for the h3 products (its max comes from the dz1
      // product's A reads: a max slot here would cost the BatchNorm backward
      // a block barrier)
      MOLCLR_TRY(seg_bn_bwd(seg, !bn_batch_stats(e), dy, z, e->bn_weight[l], e->bn_bias[l], F(lay.mean[l]),
                            F(lay.invstd[l]), dz, gr->bn_weight[l], gr->bn_bias[l], D,
                            MOLCLR_DTYPE_F32, last ? 0 : 1, 1, rdz, nullptr, drop.at(l), kws,
                            kws_bytes, stream));
    } else {
      MOLCLR_TRY(seg_bn_bwd(seg, !bn_batch_stats(e), dy, z, e->bn_weight[l], e->bn_bias[l], F(lay.mean[l]),
                            F(lay.invstd[l]), dz, gr->bn_weight[l], gr->bn_bias[l], D, dt,
                            last ? 0 : 1, 1, nullptr, nullptr, drop.at(l), kws, kws_bytes, stream));
    }
    if (bf) {
      const uint16_t *hz = (const uint16_t*)dz, *ha1 = (const uint16_t*)a1;
      // second Linear: dW2, db2 from dz and a1; dz1 = (dz W2) * (a1 > 0)
      if (gr->mlp2_weight[l] || gr->mlp2_bias[l]) {
        MOLCLR_REQUIRE(gr->mlp2_weight[l], "gin_encoder_bwd: bf16 needs the weight gradient");
        MOLCLR_TRY(molclr_linear_wgrad_bf16(hz, ha1, gr->mlp2_weight[l], gr->mlp2_bias[l], N, D,
                                            2 * D, D, 2 * D, 1, kws, kws_bytes, stream));
      }
      if (D % 64 == 0)  // the mask from the forward's bits
        MOLCLR_TRY(molclr_gemm_bf16_bits(hz, e->mlp2_planes_t[l], (uint16_t*)dz1, N, 2 * D, D, D,
                                         2 * D, MOLCLR_EPI_RELU_MASK, nullptr, nullptr,
                                         (const uint32_t*)(A + lay.bits[l]), stream));
      else
        MOLCLR_TRY(molclr_gemm_bf16(hz, e->mlp2_planes_t[l], (uint16_t*)dz1, N, 2 * D, D, D, 2 * D,
                                    MOLCLR_EPI_RELU_MASK, nullptr, ha1, 2 * D, stream));
      if (gr->mlp0_weight[l] || gr->mlp0_bias[l]) {
        MOLCLR_REQUIRE(gr->mlp0_weight[l], "gin_encoder_bwd: bf16 needs the weight gradient");
        MOLCLR_TRY(molclr_linear_wgrad_bf16((const uint16_t*)dz1, (const uint16_t*)agg,
                                            gr->mlp0_weight[l], gr->mlp0_bias[l], N, 2 * D, D,
                                            2 * D, D, 1, kws, kws_bytes, stream));
      }
      MOLCLR_TRY(molclr_gemm_bf16((const uint16_t*)dz1, e->mlp0_planes_t[l], (uint16_t*)dagg, N,
                                  D, 2 * D, 2 * D, D, MOLCLR_EPI_NONE, nullptr, nullptr, 0, stream));
      MOLCLR_TRY(molclr_gine_aggregate_bwd_bf16((const uint16_t*)dagg, g->rowptr_t, g->col_t,
                                                g->nbr_t, g->ecount, (uint16_t*)dh,
                                                gr->edge_embedding1[l], gr->edge_embedding2[l], N,
                                                D, 1, kws, kws_bytes, stream));
    } else if (h3) {
      // ops._MLP's h3 backward: dz1 (ReLU mask of a1), dW2 (+db2), dW1 (+db1),
      // dagg.  The data-gradient products scale A row by row (gradient rows
      // span many binades): dz's row maxima come from the BatchNorm backward,
      // max |dz| from the dz1 product's A reads, dz1's from its epilogue.
      const float *fz = (const float*)dz, *fa1 = (const float*)a1, *fagg = (const float*)agg;
      float* sl = bmax + 2 * l * kMaxSlotFloats;
      const float* fl = fmax + 2 * l * kMaxSlotFloats;
      MOLCLR_REQUIRE(gr->mlp2_weight[l] && gr->mlp2_bias[l] && gr->mlp0_weight[l] &&
                         gr->mlp0_bias[l],
                     "gin_encoder_bwd: h3 needs every MLP gradient");
      // dz1 (its epilogue yields dz1's max and row maxima), then the weight
      // gradients
      MOLCLR_TRY(molclr_gemm_f32_h3(fz, rdz, molclr_bn_row_parts(D), e->mlp2_planes_t[l],
                                    (float*)dz1, N, 2 * D, D, D, 2 * D, MOLCLR_EPI_RELU_MASK,
                                    nullptr, fa1, 2 * D, (const uint32_t*)(A + lay.bits[l]),
                                    sl + kMaxSlotFloats, rdz1, sl, stream));
      if (N >= 1024) {  // both weight gradients, one reduction launch
        MOLCLR_TRY(molclr_linear_wgrad_h3_pair(
            fz, sl, fa1, fl + kMaxSlotFloats, gr->mlp2_weight[l], gr->mlp2_bias[l], D, 2 * D, D,
            2 * D, (const float*)dz1, sl + kMaxSlotFloats, fagg, fl, gr->mlp0_weight[l],
            gr->mlp0_bias[l], 2 * D, D, 2 * D, D, N, 1, kws, kws_bytes, stream));
      } else {
        MOLCLR_TRY(molclr_linear_wgrad_h3(fz, sl, fa1, fl + kMaxSlotFloats, gr->mlp2_weight[l],
                                          gr->mlp2_bias[l], N, D, 2 * D, D, 2 * D, 1, kws,
                                          kws_bytes, stream));
        MOLCLR_TRY(molclr_linear_wgrad_h3((const float*)dz1, sl + kMaxSlotFloats, fagg, fl,
                                          gr->mlp0_weight[l], gr->mlp0_bias[l], N, 2 * D, D, 2 * D,
                                          D, 1, kws, kws_bytes, stream));
      }
      MOLCLR_TRY(molclr_gemm_f32_h3((const float*)dz1, rdz1, (int)molclr_gemm_row_parts(2 * D),
                                    e->mlp0_planes_t[l], (float*)dagg, N, D, 2 * D, 2 * D, D,
                                    MOLCLR_EPI_NONE, nullptr, nullptr, 0, nullptr, nullptr,
                                    nullptr, nullptr, stream));
      MOLCLR_TRY(molclr_gine_aggregate_bwd((const float*)dagg, g->rowptr_t, g->col_t, g->nbr_t,
                                           g->ecount, (float*)dh, gr->edge_embedding1[l],
                                           gr->edge_embedding2[l], N, D, 1, kws, kws_bytes, stream));
    } else {
      const float *fz = (const float*)dz, *fa1 = (const float*)a1;
      // second Linear (ops.linear_bwd order: dW with db, dx with the ReLU mask of a1)
      if (gr->mlp2_weight[l])
        MOLCLR_TRY(molclr_linear_wgrad(fz, fa1, gr->mlp2_weight[l], gr->mlp2_bias[l], N, D, 2 * D,
                                       D, 2 * D, 1, kws, kws_bytes, stream));
      else if (gr->mlp2_bias[l])
        MOLCLR_TRY(molclr_colsum_f32(fz, gr->mlp2_bias[l], N, D, D, 1, kws, kws_bytes, stream));
      MOLCLR_TRY(molclr_gemm_f32_bplanes(fz, e->mlp2_planes_t[l], (float*)dz1, N, 2 * D, D, D,
                                         2 * D, 0, MOLCLR_EPI_RELU_MASK, nullptr, fa1, 2 * D, kws,
                                         kws_bytes, stream));
      // first Linear
      if (gr->mlp0_weight[l])
        MOLCLR_TRY(molclr_linear_wgrad((const float*)dz1, (const float*)agg, gr->mlp0_weight[l],
                                       gr->mlp0_bias[l], N, 2 * D, D, 2 * D, D, 1, kws, kws_bytes,
                                       stream));
      else if (gr->mlp0_bias[l])
        MOLCLR_TRY(molclr_colsum_f32((const float*)dz1, gr->mlp0_bias[l], N, 2 * D, 2 * D, 1, kws,
                                     kws_bytes, stream));
      MOLCLR_TRY(molclr_gemm_f32_bplanes((const float*)dz1, e->mlp0_planes_t[l], (float*)dagg, N,
                                         D, 2 * D, 2 * D, D, 0, MOLCLR_EPI_NONE, nullptr, nullptr,
                                         0, kws, kws_bytes, stream));
      // aggregation: dh of the layer input, edge-table gradients
      MOLCLR_TRY(molclr_gine_aggregate_bwd((const float*)dagg, g->rowptr_t, g->col_t, g->nbr_t,
                                           g->ecount, (float*)dh, gr->edge_embedding1[l],
                                           gr->edge_embedding2[l], N, D, 1, kws, kws_bytes, stream));
    }
    MOLCLR_TRY(record_done(gr->layer_done[l], stream));
    dy = dh;
  }
  if (gr->x_embedding1 || gr->x_embedding2) {
    MOLCLR_REQUIRE(gr->x_embedding1 && gr->x_embedding2,
                   "gin_encoder_bwd: both atom-embedding grads or neither");
    if (bf)
      MOLCLR_TRY(molclr_atom_embed_bwd_bf16(x, (const uint16_t*)dh, gr->x_embedding1,
                                            gr->x_embedding2, N, D, e->n_atom, e->n_chiral, 1, kws,
                                            kws_bytes, stream));
    else
      MOLCLR_TRY(molclr_atom_embed_bwd(x, (const float*)dh, gr->x_embedding1, gr->x_embedding2, N,
                                       D, e->n_atom, e->n_chiral, 1, kws, kws_bytes, stream));
  }
  MOLCLR_TRY(record_done(gr->embed_done, stream));
  return MOLCLR_OK;
}

// ---------------------------------------------------------------------------
// GCN encoder executor (models/gcn_molclr.py:140-151), same scheme: per layer
// xw = x W (scratch), z = gcn_aggregate(xw) + bias (BatchNorm input, saved),
// h = BatchNorm(z) (+ReLU but the last; the next layer's input, saved).
// Arena: per layer z_l, h_l [N,D] in the encoder's storage type, mean_l /
// invstd_l [D] fp32; then h0 [N,D] and the dropout key (as the GIN executor's).
// Workspace: xw / dxw, dz, dh [N,D] x 3 in the storage type, then the entry
// points' largest.
// bf16 storage (dtype MOLCLR_DTYPE_BF16): one bf16 MFMA per product on plane 0
// of the same weight images, the bf16 aggregation, BatchNorm and weight
// gradient; no h3 form.
// ---------------------------------------------------------------------------
namespace {

// byte offsets, every buffer 256-byte aligned; es: bytes of a node-feature element
struct GcnArena {
  size_t z[MOLCLR_MAX_LAYERS], h[MOLCLR_MAX_LAYERS], mean[MOLCLR_MAX_LAYERS],
      invstd[MOLCLR_MAX_LAYERS];
  size_t hmax[MOLCLR_MAX_LAYERS];  // h3: max slot of layer l's input (contiguous)
  size_t h0, dropkey, total;  // dropkey: this forward's dropout key (seed, call)
  GcnArena(int L, int64_t N, int64_t D, size_t es) {
    size_t used = 0;
    auto off = [&](size_t bytes) {
      const size_t o = used;
      used += (bytes + 255) / 256 * 256;
      return o;
    };
    for (int l = 0; l < L; ++l) {
      z[l] = off(N * D * es);
      h[l] = off(N * D * es);
      mean[l] = off(MOLCLR_MAX_SEGMENTS * D * sizeof(float));  // [segment][D]
      invstd[l] = off(MOLCLR_MAX_SEGMENTS * D * sizeof(float));
    }
    const size_t slots = off((size_t)L * kMaxSlotFloats * sizeof(float));
    for (int l = 0; l < L; ++l) hmax[l] = slots + (size_t)l * kMaxSlotFloats * sizeof(float);
    h0 = off(N * D * es);
    dropkey = off(2 * sizeof(int64_t));
    total = used;
  }
};

size_t gcn_kernels_ws(int64_t N, int64_t D, int dtype) {
  size_t m = 0;
  auto mx = [&](size_t v) { m = v > m ? v : m; };
  mx(molclr_gemm_f32_workspace_bytes(N, D, D));  // x W, dxw W^T
  mx(molclr_gemm_f32_workspace_bytes(D, D, N));  // dW = x^T dxw
  mx(molclr_linear_wgrad_workspace_bytes(N, D, D));  // its h3 form
  if (dtype == MOLCLR_DTYPE_BF16) mx(molclr_linear_wgrad_bf16_workspace_bytes(N, D, D));
  mx(molclr_batchnorm_ws_bound(N, D));
  mx(molclr_gcn_aggregate_bwd_workspace_bytes(N, D));
  mx(molclr_atom_embed_bwd_workspace_bytes(N, D, MOLCLR_NUM_ATOM_TYPE, MOLCLR_NUM_CHIRALITY));
  return m;
}
// xw / dxw, dz, dh [N,D] in the storage type
size_t gcn_scratch_bytes(int64_t N, int64_t D, size_t es) { return (size_t)N * D * 3 * es; }
// h3 backward: dxw's row maxima [N] and max slot, after the scratch
size_t gcn_h3_bytes(int64_t N) {
  return molclr::align_up((size_t)N * sizeof(float), 256) + kMaxSlotFloats * sizeof(float);
}
bool gcn_dtype_ok(int dtype) { return dtype == MOLCLR_DTYPE_F32 || dtype == MOLCLR_DTYPE_BF16; }

int check_gcn(const molclr_gcn_encoder* e, const molclr_device_graph* g) {
  MOLCLR_REQUIRE(e && g, "gcn_encoder: null encoder / graph");
  MOLCLR_TRY_RC(check_drop("gcn_encoder", e->drop_ratio, e->drop_state, e->training));
  MOLCLR_REQUIRE(e->num_layer >= 1 && e->num_layer <= MOLCLR_MAX_LAYERS,
                 "gcn_encoder: num_layer %d", e->num_layer);
  MOLCLR_REQUIRE(e->dim > 0 && e->dim % 4 == 0, "gcn_encoder: dim %lld", (long long)e->dim);
  MOLCLR_REQUIRE(e->dtype == MOLCLR_DTYPE_F32 || (e->dtype == MOLCLR_DTYPE_BF16 && e->dim % 8 == 0),
                 "gcn_encoder: dtype %d (bf16 needs dim %% 8 == 0)", e->dtype);
  MOLCLR_REQUIRE(e->dtype == MOLCLR_DTYPE_F32 || e->fp32_gemm == 0,
                 "gcn_encoder: fp32_gemm %d with bf16 storage", e->fp32_gemm);
  MOLCLR_REQUIRE(e->n_atom == MOLCLR_NUM_ATOM_TYPE && e->n_chiral == MOLCLR_NUM_CHIRALITY,
                 "gcn_encoder: embedding tables must be [%d,D] and [%d,D]",
                 MOLCLR_NUM_ATOM_TYPE, MOLCLR_NUM_CHIRALITY);
  for (int l = 0; l < e->num_layer; ++l)
    MOLCLR_REQUIRE(e->weight_planes[l] && e->weight_planes_t[l] && e->bias[l] &&
                       e->edge_embedding1[l] && e->edge_embedding2[l] && e->bn_weight[l] &&
                       e->bn_bias[l],
                   "gcn_encoder: layer %d: missing planes, bias, edge tables or BatchNorm", l);
  return MOLCLR_OK;
}

}  // namespace

MOLCLR_API size_t molclr_gcn_encoder_arena_bytes_dtype(int L, int64_t N, int64_t D, int dtype) {
  if (L < 1 || L > MOLCLR_MAX_LAYERS || !gcn_dtype_ok(dtype)) return 0;
  return GcnArena(L, N, D, elem_bytes(dtype)).total;
}

MOLCLR_API size_t molclr_gcn_encoder_workspace_bytes_dtype(int L, int64_t N, int64_t D,
                                                           int dtype) {
  (void)L;
  if (!gcn_dtype_ok(dtype)) return 0;
  return gcn_scratch_bytes(N, D, elem_bytes(dtype)) + 256 + gcn_h3_bytes(N) +
         gcn_kernels_ws(N, D, dtype) + 256;
}

MOLCLR_API size_t molclr_gcn_encoder_arena_bytes(int L, int64_t N, int64_t D) {
  return molclr_gcn_encoder_arena_bytes_dtype(L, N, D, MOLCLR_DTYPE_F32);
}

MOLCLR_API size_t molclr_gcn_encoder_workspace_bytes(int L, int64_t N, int64_t D) {
  return molclr_gcn_encoder_workspace_bytes_dtype(L, N, D, MOLCLR_DTYPE_F32);
}

MOLCLR_API int molclr_gcn_encoder_fwd(const molclr_gcn_encoder* e, const int64_t* x,
                                      const molclr_device_graph* g, void* h_out, void* arena,
                                      size_t arena_bytes, void* workspace, size_t workspace_bytes,
                                      molclr_stream_t stream) {
  MOLCLR_TRY(check_gcn(e, g));
  const int L = e->num_layer;
  const int64_t N = g->num_nodes, D = e->dim;
  if (N == 0) return MOLCLR_OK;
  SegRows seg;
  MOLCLR_TRY(graph_segments(g, &g->num_nodes, seg));
  MOLCLR_REQUIRE(x && h_out && arena, "gcn_encoder_fwd: null pointer");
  const bool bf = e->dtype == MOLCLR_DTYPE_BF16;
  const size_t es = elem_bytes(e->dtype);
  const GcnArena lay(L, N, D, es);
  MOLCLR_REQUIRE_WS(arena_bytes, lay.total);
  MOLCLR_REQUIRE_WS(workspace_bytes, molclr_gcn_encoder_workspace_bytes_dtype(L, N, D, e->dtype));
  char* A = (char*)arena;
  auto F = [&](size_t off) { return (float*)(A + off); };
  void* xw = workspace;
  void* kws = (char*)workspace + molclr::align_up(gcn_scratch_bytes(N, D, es), 256);
  const size_t kws_bytes = gcn_kernels_ws(N, D, e->dtype);

  const bool h3 = e->fp32_gemm == 1;
  if (h3 && molclr::zero_async(A + lay.hmax[0], (size_t)L * kMaxSlotFloats * sizeof(float),
                           molclr::as_stream(stream)) != hipSuccess) {
    molclr::set_error("gcn_encoder_fwd: zeroing the max slots failed");
    return MOLCLR_ERR_ARG;
  }
  CallDrop drop(e->training, e->drop_ratio, A + lay.dropkey);
  MOLCLR_TRY(open_drop(drop, e->drop_state, stream));
  void* h = A + lay.h0;
  if (bf)
    MOLCLR_TRY(molclr_atom_embed_fwd_bf16(x, e->x_embedding1, e->x_embedding2, (uint16_t*)h, N, D,
                                          e->n_atom, e->n_chiral, e->status, stream));
  else
    MOLCLR_TRY(molclr_atom_embed_fwd(x, e->x_embedding1, e->x_embedding2, (float*)h, N, D,
                                     e->n_atom, e->n_chiral, e->status, stream));
  for (int l = 0; l < L; ++l) {
    void* z = A + lay.z[l];
    const bool last = l == L - 1;
    void* y = last ? h_out : A + lay.h[l];
    // x W, W [in, out] as a K-major B (ops.gemm_w(x, W, N, D, D, D, D, False, True))
    if (bf) {  // plane 0 of the same image: bf16(W), one MFMA per product
      MOLCLR_TRY(molclr_gemm_bf16((const uint16_t*)h, e->weight_planes[l], (uint16_t*)xw, N, D, D,
                                  D, D, MOLCLR_EPI_NONE, nullptr, nullptr, 0, stream));
      MOLCLR_TRY(molclr_gcn_aggregate_fwd_bf16((const uint16_t*)xw, g->rowptr, g->col, g->ecode,
                                               g->nbr, e->edge_embedding1[l],
                                               e->edge_embedding2[l], e->bias[l], (uint16_t*)z, N,
                                               D, stream));
    } else {
      if (h3)  // the same product, also folding max |h| into the layer's slot
        MOLCLR_TRY(molclr_gemm_f32_bplanes_max((const float*)h, e->weight_planes[l], (float*)xw, N,
                                               D, D, D, D, MOLCLR_EPI_NONE, nullptr, nullptr, 0,
                                               F(lay.hmax[l]), nullptr, nullptr, nullptr, kws,
                                               kws_bytes, stream));
      else
        MOLCLR_TRY(molclr_gemm_f32_bplanes((const float*)h, e->weight_planes[l], (float*)xw, N, D,
                                           D, D, D, 0, MOLCLR_EPI_NONE, nullptr, nullptr, 0, kws,
                                           kws_bytes, stream));
      MOLCLR_TRY(molclr_gcn_aggregate_fwd((const float*)xw, g->rowptr, g->col, g->ecode, g->nbr,
                                          e->edge_embedding1[l], e->edge_embedding2[l], e->bias[l],
                                          (float*)z, N, D, stream));
    }
    MOLCLR_TRY(seg_bn_fwd(seg, z, e->bn_weight[l], e->bn_bias[l], e->bn_running_mean[l],
                          e->bn_running_var[l], e->bn_num_batches_tracked[l], y, F(lay.mean[l]),
                          F(lay.invstd[l]), D, e->dtype, e->momentum, e->eps, bn_batch_stats(e),
                          last ? 0 : 1, drop.at(l), kws, kws_bytes, stream));
    h = y;
  }
  return MOLCLR_OK;
}

MOLCLR_API int molclr_gcn_encoder_bwd(const molclr_gcn_encoder* e,
                                      const molclr_gcn_encoder_grads* gr, const int64_t* x,
                                      const molclr_device_graph* g, const void* dh_out,
                                      const void* arena, size_t arena_bytes, void* workspace,
                                      size_t workspace_bytes, molclr_stream_t stream) {
  MOLCLR_TRY(check_gcn(e, g));
  MOLCLR_REQUIRE(gr, "gcn_encoder_bwd: null grads");
  const int L = e->num_layer;
  const int64_t N = g->num_nodes, D = e->dim;
  if (N == 0) return MOLCLR_OK;
  SegRows seg;
  MOLCLR_TRY(graph_segments(g, &g->num_nodes, seg));
  MOLCLR_REQUIRE(x && dh_out && arena, "gcn_encoder_bwd: null pointer");
  const bool bf = e->dtype == MOLCLR_DTYPE_BF16;
  const size_t es = elem_bytes(e->dtype);
  const GcnArena lay(L, N, D, es);
  MOLCLR_REQUIRE_WS(arena_bytes, lay.total);
  MOLCLR_REQUIRE_WS(workspace_bytes, molclr_gcn_encoder_workspace_bytes_dtype(L, N, D, e->dtype));
  const char* A = (const char*)arena;
  auto F = [&](size_t off) { return (const float*)(A + off); };
  char* S = (char*)workspace;
  void* dxw = S;
  void* dz = S + (size_t)N * D * es;
  void* dh = S + 2 * (size_t)N * D * es;
  // h3: dxw's row maxima and max slot
  float* rdxw = (float*)(S + molclr::align_up(gcn_scratch_bytes(N, D, es), 256));
  float* sdxw = (float*)((char*)rdxw + molclr::align_up((size_t)N * sizeof(float), 256));
  void* kws = (char*)rdxw + gcn_h3_bytes(N);
  const size_t kws_bytes = gcn_kernels_ws(N, D, e->dtype);
  const bool h3 = e->fp32_gemm == 1;
  CallDrop drop(e->training, e->drop_ratio, A + lay.dropkey);  // the forward's key

  const void* dy = dh_out;
  for (int l = L - 1; l >= 0; --l) {
    const void* z = A + lay.z[l];
    const void* xin = l == 0 ? A + lay.h0 : A + lay.h[l - 1];
    const bool last = l == L - 1;
    MOLCLR_REQUIRE(gr->bn_weight[l] && gr->bn_bias[l], "gcn_encoder_bwd: BatchNorm grads needed");
    MOLCLR_TRY(seg_bn_bwd(seg, !bn_batch_stats(e), dy, z, e->bn_weight[l], e->bn_bias[l], F(lay.mean[l]),
                          F(lay.invstd[l]), dz, gr->bn_weight[l], gr->bn_bias[l], D, e->dtype,
                          last ? 0 : 1, 1, nullptr, nullptr, drop.at(l), kws, kws_bytes, stream));
    // ops._GCNConv.backward order: aggregation (dxw, edge tables, bias), dW, dx
    if (bf) {
      MOLCLR_TRY(molclr_gcn_aggregate_bwd_bf16((const uint16_t*)dz, g->rowptr_t, g->col_t,
                                               g->nbr_t, g->ecount, (uint16_t*)dxw,
                                               gr->edge_embedding1[l], gr->edge_embedding2[l],
                                               gr->bias[l], N, D, 1, kws, kws_bytes, stream));
      // dW [in, out] += x^T dxw: x in the dy slot, dxw in the x slot, no bias sum
      if (gr->weight[l])
        MOLCLR_TRY(molclr_linear_wgrad_bf16((const uint16_t*)xin, (const uint16_t*)dxw,
                                            gr->weight[l], nullptr, N, D, D, D, D, 1, kws,
                                            kws_bytes, stream));
      MOLCLR_TRY(molclr_gemm_bf16((const uint16_t*)dxw, e->weight_planes_t[l], (uint16_t*)dh, N, D,
                                  D, D, D, MOLCLR_EPI_NONE, nullptr, nullptr, 0, stream));
    } else {
      const float* fxin = (const float*)xin;
      float *fdxw = (float*)dxw, *fdh = (float*)dh;
      MOLCLR_TRY(molclr_gcn_aggregate_bwd((const float*)dz, g->rowptr_t, g->col_t, g->nbr_t,
                                          g->ecount, fdxw, gr->edge_embedding1[l],
                                          gr->edge_embedding2[l], gr->bias[l], N, D, 1, kws,
                                          kws_bytes, stream));
      if (h3) {
        // ops._GCNConv's h3 backward: dxw's row maxima / max, dW = x^T dxw
        // (per-tensor scales), dx = dxw W^T (row-wise)
        MOLCLR_TRY(molclr_absmax_rows_f32(fdxw, N, D, D, rdxw, sdxw, 0, stream));
        if (gr->weight[l])
          MOLCLR_TRY(molclr_linear_wgrad_h3(fxin, F(lay.hmax[l]), fdxw, sdxw, gr->weight[l],
                                            nullptr, N, D, D, D, D, 1, kws, kws_bytes, stream));
        MOLCLR_TRY(molclr_gemm_f32_h3(fdxw, rdxw, 1, e->weight_planes_t[l], fdh, N, D, D, D, D,
                                      MOLCLR_EPI_NONE, nullptr, nullptr, 0, nullptr, nullptr,
                                      nullptr, nullptr, stream));
      } else {
        if (gr->weight[l])  // dW [in, out] = x^T dxw
          MOLCLR_TRY(molclr_gemm_f32(fxin, fdxw, gr->weight[l], D, D, N, D, D, D, 1, 1,
                                     MOLCLR_EPI_NONE | MOLCLR_EPI_ACCUMULATE, nullptr, nullptr, 0,
                                     kws, kws_bytes, stream));
        // dx = dxw W^T  (ops.gemm_w(dxw, W, N, D, D, D, D, False, False))
        MOLCLR_TRY(molclr_gemm_f32_bplanes(fdxw, e->weight_planes_t[l], fdh, N, D, D, D, D, 0,
                                           MOLCLR_EPI_NONE, nullptr, nullptr, 0, kws, kws_bytes,
                                           stream));
      }
    }
    MOLCLR_TRY(record_done(gr->layer_done[l], stream));
    dy = dh;
  }
  if (gr->x_embedding1 || gr->x_embedding2) {
    MOLCLR_REQUIRE(gr->x_embedding1 && gr->x_embedding2,
                   "gcn_encoder_bwd: both atom-embedding grads or neither");
    if (bf)
      MOLCLR_TRY(molclr_atom_embed_bwd_bf16(x, (const uint16_t*)dh, gr->x_embedding1,
                                            gr->x_embedding2, N, D, e->n_atom, e->n_chiral, 1, kws,
                                            kws_bytes, stream));
    else
      MOLCLR_TRY(molclr_atom_embed_bwd(x, (const float*)dh, gr->x_embedding1, gr->x_embedding2, N,
                                       D, e->n_atom, e->n_chiral, 1, kws, kws_bytes, stream));
  }
  MOLCLR_TRY(record_done(gr->embed_done, stream));
  return MOLCLR_OK;
}
