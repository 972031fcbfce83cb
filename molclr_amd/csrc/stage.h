// Staging of a batch into a captured step's fixed-capacity buffers: the one
// launch that runs outside the captured region (molclr_stage_segments in
// graph.hip, molclr_stage_task in finetune_step.hip).
#pragma once

#include "common.h"

namespace molclr {

constexpr int kStageJobs = 5 * MOLCLR_MAX_SEGMENTS + 1;
struct StageJob {
  const int64_t* src;  // NULL: fill with 0
  int64_t* dst;
  int64_t count;
};
struct StageJobs {
  StageJob j[kStageJobs];
  int64_t counts[2 * MOLCLR_MAX_SEGMENTS];
  int64_t* counts_dst;
  int ncounts;
  // a further copy in 4-byte words (a task's targets: fp32 values, or int64
  // labels as word pairs); nwords = 0 without one
  const uint32_t* words_src;
  uint32_t* words_dst;
  int64_t nwords;
};

// blockIdx.y: the job; grid-stride over its elements.  The words go with job 0.
__global__ static void k_stage(StageJobs jb) {
  const StageJob& j = jb.j[blockIdx.y];
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = t0; i < j.count; i += stride) j.dst[i] = j.src ? j.src[i] : 0;
  if (blockIdx.y == 0)
    for (int64_t i = t0; i < jb.nwords; i += stride) jb.words_dst[i] = jb.words_src[i];
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < jb.ncounts)
    jb.counts_dst[threadIdx.x] = jb.counts[threadIdx.x];
}

// The jobs of nseg segments (see molclr_stage_segments in molclr.h) into jb;
// refuses what the capacities do not hold before anything is launched.
inline int stage_plan(const char* who, int nseg, const molclr_stage_source* src,
                      const molclr_graph_staged_segment* dst, int64_t* x_all,
                      int64_t num_nodes_cap, int64_t num_edges_cap, int64_t* counts, StageJobs& jb,
                      int& nj, int64_t& most) {
  if (!(nseg >= 1 && nseg <= MOLCLR_MAX_SEGMENTS && src && dst && x_all && counts)) {
    set_error("%s: %d segments (1..%d) / null pointer", who, nseg, MOLCLR_MAX_SEGMENTS);
    return MOLCLR_ERR_ARG;
  }
  nj = 0;
  most = 1;
  int64_t row = 0, edges = 0;
  auto job = [&](const int64_t* from, int64_t* to, int64_t n) {
    jb.j[nj++] = {from, to, n};
    if (n > most) most = n;
  };
  for (int s = 0; s < nseg; ++s) {
    const molclr_stage_source& a = src[s];
    const molclr_graph_staged_segment& b = dst[s];
    if (!(a.num_nodes >= 0 && a.num_edges >= 0 && a.num_nodes <= b.node_cap &&
          a.num_edges <= b.edge_cap)) {
      set_error("%s: segment %d has %lld nodes / %lld edges, capacity %lld / %lld", who, s,
                (long long)a.num_nodes, (long long)a.num_edges, (long long)b.node_cap,
                (long long)b.edge_cap);
      return MOLCLR_ERR_ARG;
    }
    if (!((a.num_nodes == 0 || (a.x && a.batch && b.batch)) &&
          (a.num_edges == 0 || (a.edge_index && a.edge_attr && b.edge_index && b.edge_attr)))) {
      set_error("%s: null buffer in segment %d", who, s);
      return MOLCLR_ERR_ARG;
    }
    job(a.x, x_all + 2 * row, 2 * a.num_nodes);
    job(a.edge_index, const_cast<int64_t*>(b.edge_index), a.num_edges);
    job(a.edge_index + a.num_edges, const_cast<int64_t*>(b.edge_index) + b.edge_cap, a.num_edges);
    job(a.edge_attr, const_cast<int64_t*>(b.edge_attr), 2 * a.num_edges);
    job(a.batch, const_cast<int64_t*>(b.batch), a.num_nodes);
    jb.counts[s] = a.num_nodes;
    jb.counts[nseg + s] = a.num_edges;
    row += a.num_nodes;
    edges += a.num_edges;
  }
  if (edges > num_edges_cap) {
    set_error("%s: %lld edges exceed the capacity %lld", who, (long long)edges,
              (long long)num_edges_cap);
    return MOLCLR_ERR_ARG;
  }
  if (row > num_nodes_cap) {
    set_error("%s: %lld nodes exceed the capacity %lld", who, (long long)row,
              (long long)num_nodes_cap);
    return MOLCLR_ERR_ARG;
  }
  job(nullptr, x_all + 2 * row, 2 * (num_nodes_cap - row));  // padding atoms: type 0, chirality 0
  jb.counts_dst = counts;
  jb.ncounts = 2 * nseg;
  return MOLCLR_OK;
}

inline void stage_launch(const StageJobs& jb, int nj, int64_t most, hipStream_t stream) {
  const int T = 256;
  int64_t bx = ceil_div(most, T);
  if (bx > 256) bx = 256;
  hipLaunchKernelGGL(k_stage, dim3((unsigned)bx, nj), dim3(T), 0, stream, jb);
}

}  // namespace molclr
