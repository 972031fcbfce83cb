// On-device collate of labelled molecules for fine-tuning: the counterpart of
// augment.hip's node-mask views for dataset_test.py's MolTestDataset and its
// DataLoader (dataset_test.py:114-169 per molecule, PyG's Batch.from_data_list
// per batch).  The molecules live in HBM in the molclr_mask_views store,
// featurised once, next to a target table; a batch is its molecule ids.
//   molclr_collate_task     the Batch fields and the gathered targets (eager)
//   molclr_stage_task_ids   the same gather straight into the fixed buffers
//                           molclr_stage_task fills (the captured steps)
//   molclr_motif_items      the motif model's (mol_idx, clique_idx) of a batch
//                           from the resident motif CSR (eager)
//   molclr_stage_motif_ids  those items into the buffers molclr_stage_motif
//                           fills, by the same staging kernel
// Shape: a gather of 16-byte records (an x row and an edge_attr row are two
// int64).  One block scans the batch's atom / edge counts into offsets (wave
// scans by shuffles, the waves' totals through LDS), then one wave per
// molecule copies its records with strided loops -- a molecule of any size is
// correct, and molecule k's rows precede molecule k + 1's exactly.  No atomics
// besides the status word's OR.
#include "common.h"
#include "stage.h"

namespace {

constexpr int kMolsPerBlock = 4;  // one wave per molecule
constexpr int kScanMax = 1024;    // threads of the scan block
constexpr int kExpandThreads = 256;

typedef int64_t rec16 __attribute__((ext_vector_type(2)));  // one 16-byte record

// threads of the one-block scan over B entries: whole waves, no idle ones
inline int scan_threads(int64_t B) {
  const int64_t t = molclr::ceil_div(B > 0 ? B : 1, 64) * 64;
  return (int)(t < kScanMax ? t : kScanMax);
}

// Exclusive scan of (a, e) over the block's threads; tot_*: the block's sums.
// s_a / s_e: LDS, one entry per wave.  Every thread of the block must call it.
__device__ __forceinline__ void block_scan2(int64_t a, int64_t e, int64_t* s_a, int64_t* s_e,
                                            int64_t& ex_a, int64_t& ex_e, int64_t& tot_a,
                                            int64_t& tot_e) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  int64_t ia = a, ie = e;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t ua = __shfl_up(ia, o, 64), ue = __shfl_up(ie, o, 64);
    if (lane >= o) {
      ia += ua;
      ie += ue;
    }
  }
  if (lane == 63) {
    s_a[w] = ia;
    s_e[w] = ie;
  }
  __syncthreads();
  int64_t ba = 0, be = 0;
  tot_a = 0;
  tot_e = 0;
  for (int q = 0; q < nw; ++q) {
    const int64_t va = s_a[q], ve = s_e[q];
    if (q < w) {
      ba += va;
      be += ve;
    }
    tot_a += va;
    tot_e += ve;
  }
  __syncthreads();  // s_a / s_e are rewritten by the next chunk
  ex_a = ba + ia - a;
  ex_e = be + ie - e;
}

struct TaskOffsets {
  const int64_t *atom_ptr, *bond_ptr, *mol_ids;
  int64_t B, G;
  int64_t *ptr, *edge_off;       // [B + 1] each
  int64_t num_nodes, num_edges;  // the host's sums
  int32_t* status;
  int64_t* counts;  // staged form: [2] = (nodes, edges), (0, 0) on a mismatch; else NULL
  const void* target_table;  // int64 [G] or fp32 [G, cols]
  void* target_out;          // int64 [B] or fp32 [B, cols]
  int64_t cols;
  int target_is_float;
};

// pass 1, one block: ptr (atom offsets, the Batch's ptr), edge offsets, the
// gathered targets, the status word's bits 0 and 1
__global__ __launch_bounds__(kScanMax) void k_task_offsets(TaskOffsets a) {
  __shared__ int64_t s_a[kScanMax / 64], s_e[kScanMax / 64];
  const int t = threadIdx.x;
  if (t == 0) *a.status = 0;
  __syncthreads();
  int bad = 0;
  int64_t carry_a = 0, carry_e = 0;  // the same in every thread
  for (int64_t base = 0; base < a.B; base += blockDim.x) {
    const int64_t b = base + t;
    int64_t n = 0, e = 0, id = -1;
    if (b < a.B) {
      id = a.mol_ids[b];
      if (id < 0 || id >= a.G) {
        bad |= 1;
        id = -1;
      } else {
        n = a.atom_ptr[id + 1] - a.atom_ptr[id];
        e = 2 * (a.bond_ptr[id + 1] - a.bond_ptr[id]);
      }
    }
    int64_t ex_a, ex_e, tot_a, tot_e;
    block_scan2(n, e, s_a, s_e, ex_a, ex_e, tot_a, tot_e);
    if (b < a.B) {
      a.ptr[b] = carry_a + ex_a;
      a.edge_off[b] = carry_e + ex_e;
      // the molecule's targets; a refused id's row is 0
      if (a.target_is_float) {
        const float* src = static_cast<const float*>(a.target_table);
        float* dst = static_cast<float*>(a.target_out);
        for (int64_t c = 0; c < a.cols; ++c)
          dst[b * a.cols + c] = id >= 0 ? src[id * a.cols + c] : 0.f;
      } else {
        static_cast<int64_t*>(a.target_out)[b] =
            id >= 0 ? static_cast<const int64_t*>(a.target_table)[id] : 0;
      }
    }
    carry_a += tot_a;
    carry_e += tot_e;
  }
  if (t == 0) {
    a.ptr[a.B] = carry_a;
    a.edge_off[a.B] = carry_e;
    const bool match = carry_a == a.num_nodes && carry_e == a.num_edges;
    if (!match) bad |= 2;
    if (a.counts) {
      a.counts[0] = match ? carry_a : 0;
      a.counts[1] = match ? carry_e : 0;
    }
  }
  if (bad) atomicOr(a.status, bad);
}

// pass 2: one wave per molecule copies its atoms and directed edges; blocks
// from mol_blocks on zero the x rows [pad_begin, pad_end) (the staged form's
// padding atoms: type 0, chirality 0).  ei_stride: elements between the two
// edge_index rows (num_edges, or the staged segment's edge_cap).
__global__ __launch_bounds__(64 * kMolsPerBlock) void k_task_gather(
    const int64_t* __restrict__ sx, const int64_t* __restrict__ atom_ptr,
    const int64_t* __restrict__ sei, const int64_t* __restrict__ sea,
    const int64_t* __restrict__ bond_ptr, int64_t store_edges, const int64_t* __restrict__ mol_ids,
    int64_t B, int64_t G, const int64_t* __restrict__ ptr, const int64_t* __restrict__ edge_off,
    int64_t* __restrict__ x_out, int64_t* __restrict__ ei_out, int64_t ei_stride,
    int64_t* __restrict__ ea_out, int64_t* __restrict__ batch_out, int64_t num_nodes,
    int64_t num_edges, int32_t* __restrict__ status, int64_t mol_blocks, int64_t pad_begin,
    int64_t pad_end) {
  rec16* x16 = reinterpret_cast<rec16*>(x_out);
  if ((int64_t)blockIdx.x >= mol_blocks) {
    const int64_t stride = ((int64_t)gridDim.x - mol_blocks) * blockDim.x;
    const rec16 zero = {0, 0};
    for (int64_t i = pad_begin + ((int64_t)blockIdx.x - mol_blocks) * blockDim.x + threadIdx.x;
         i < pad_end; i += stride)
      x16[i] = zero;
    return;
  }
  const int lane = threadIdx.x & 63;
  const int64_t b = (int64_t)blockIdx.x * kMolsPerBlock + (threadIdx.x >> 6);
  if (b >= B) return;  // wave-uniform
  const int64_t id = mol_ids[b];
  if (id < 0 || id >= G) return;  // flagged by k_task_offsets
  const int64_t a0 = atom_ptr[id], n = atom_ptr[id + 1] - a0;
  const int64_t e0 = 2 * bond_ptr[id], ne = 2 * bond_ptr[id + 1] - e0;
  const int64_t aoff = ptr[b], eoff = edge_off[b];
  // the totals were checked against the host's sizes; these guards keep a
  // mismatched call inside the outputs
  if (n < 0 || ne < 0 || aoff < 0 || eoff < 0 || aoff + n > num_nodes || eoff + ne > num_edges)
    return;
  const rec16* sx16 = reinterpret_cast<const rec16*>(sx);
  for (int64_t i = lane; i < n; i += 64) {
    x16[aoff + i] = sx16[a0 + i];
    batch_out[aoff + i] = b;
  }
  const rec16* sea16 = reinterpret_cast<const rec16*>(sea);
  rec16* ea16 = reinterpret_cast<rec16*>(ea_out);
  const int64_t top = n > 0 ? n - 1 : 0;
  int bad = 0;
  for (int64_t i = lane; i < ne; i += 64) {
    int64_t s = sei[e0 + i], t = sei[store_edges + e0 + i];
    if (s < 0 || s >= n || t < 0 || t >= n) {
      bad = 4;
      s = s < 0 ? 0 : (s > top ? top : s);
      t = t < 0 ? 0 : (t > top ? top : t);
    }
    ei_out[eoff + i] = s + aoff;
    ei_out[ei_stride + eoff + i] = t + aoff;
    ea16[eoff + i] = sea16[e0 + i];
  }
  if (bad) atomicOr(status, bad);
}

// ---- motif items --------------------------------------------------------------
// pass 1, one block: item offsets of the batch's molecules; flags[0] = the
// status bits (0: molecule id out of range, 1: the host's T is not the sum)
__global__ __launch_bounds__(kScanMax) void k_motif_offsets(
    const int64_t* __restrict__ motif_ptr, int64_t G, const int64_t* __restrict__ mol_ids,
    int64_t B, int64_t T, int64_t* __restrict__ item_off, int32_t* __restrict__ flags,
    int32_t* status) {
  __shared__ int64_t s_a[kScanMax / 64], s_e[kScanMax / 64];
  __shared__ int32_t s_bad;
  const int t = threadIdx.x;
  if (t == 0) s_bad = 0;
  __syncthreads();
  int bad = 0;
  int64_t carry = 0;
  for (int64_t base = 0; base < B; base += blockDim.x) {
    const int64_t b = base + t;
    int64_t c = 0;
    if (b < B) {
      const int64_t id = mol_ids[b];
      if (id < 0 || id >= G) {
        bad |= 1;
      } else {
        c = motif_ptr[id + 1] - motif_ptr[id];
        if (c < 0) {  // a CSR that does not ascend
          c = 0;
          bad |= 2;
        }
      }
    }
    int64_t ex, ex2, tot, tot2;
    block_scan2(c, 0, s_a, s_e, ex, ex2, tot, tot2);
    if (b < B) item_off[b] = carry + ex;
    carry += tot;
  }
  if (t == 0) {
    item_off[B] = carry;
    if (carry != T) bad |= 2;
  }
  if (bad) atomicOr(&s_bad, bad);
  __syncthreads();
  if (t == 0) {
    flags[0] = s_bad;
    if (status) *status = s_bad;
  }
}

// pass 2: thread p owns item p -- its molecule by binary search over the
// offsets, its id from the CSR -- or, from T on, the molecules' own rows
// 0 .. B - 1.  Refused items (flags[0]): the own rows are -1, which
// molclr_stage_motif's check answers with MOLCLR_STATUS_ITEM_MOL.
__global__ __launch_bounds__(kExpandThreads) void k_motif_expand(
    const int64_t* __restrict__ motif_ptr, const int64_t* __restrict__ motif_ids,
    const int64_t* __restrict__ mol_ids, int64_t B, int64_t T,
    const int64_t* __restrict__ item_off, const int32_t* __restrict__ flags,
    int64_t* __restrict__ mol_idx, int64_t* __restrict__ clique_idx) {
  const int64_t p = (int64_t)blockIdx.x * kExpandThreads + threadIdx.x;
  if (p >= T + B) return;
  if (p >= T) {
    mol_idx[p] = flags[0] ? -1 : p - T;
    return;
  }
  int64_t lo = 0, hi = B;  // the molecule b with item_off[b] <= p < item_off[b + 1]
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (item_off[mid + 1] <= p) lo = mid + 1; else hi = mid;
  }
  if (lo >= B) {  // fewer items on the device than the host counted (flagged)
    mol_idx[p] = B - 1;
    clique_idx[p] = MOLCLR_MOTIF_PAD;
    return;
  }
  const int64_t id = mol_ids[lo];  // in range: the molecule has items
  mol_idx[p] = lo;
  clique_idx[p] = motif_ids[motif_ptr[id] + (p - item_off[lo])];
}

struct TaskWs {
  int64_t *ptr, *edge_off;
};
TaskWs task_ws(void* w, size_t bytes, int64_t B) {
  molclr::Workspace ws(w, bytes);
  TaskWs a;
  a.ptr = ws.take<int64_t>(B + 1);
  a.edge_off = ws.take<int64_t>(B + 1);
  return a;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

int store_args_ok(const char* who, const int64_t* store_x, const int64_t* store_atom_ptr,
                  const int64_t* store_edge_index, const int64_t* store_edge_attr,
                  const int64_t* store_bond_ptr, int64_t store_mols, int64_t store_edges,
                  const int64_t* mol_ids, int64_t batch_size, int64_t num_nodes,
                  int64_t num_edges) {
  if (!(batch_size >= 0 && batch_size < ((int64_t)1 << 31) && store_mols >= 0 &&
        store_edges >= 0 && num_nodes >= 0 && num_edges >= 0)) {
    molclr::set_error("%s: negative size / batch too large", who);
    return MOLCLR_ERR_ARG;
  }
  if (!((batch_size == 0 || (store_atom_ptr && store_bond_ptr && mol_ids)) &&
        (num_nodes == 0 || store_x) &&
        (num_edges == 0 || (store_edge_index && store_edge_attr)))) {
    molclr::set_error("%s: null pointer", who);
    return MOLCLR_ERR_ARG;
  }
  if (!(aligned16(store_x) && aligned16(store_edge_attr))) {
    molclr::set_error("%s: store x / edge_attr must be 16-byte aligned", who);
    return MOLCLR_ERR_ARG;
  }
  return MOLCLR_OK;
}

void launch_gather(const int64_t* store_x, const int64_t* store_atom_ptr,
                   const int64_t* store_edge_index, const int64_t* store_edge_attr,
                   const int64_t* store_bond_ptr, int64_t store_mols, int64_t store_edges,
                   const int64_t* mol_ids, int64_t B, const int64_t* ptr, const int64_t* edge_off,
                   int64_t* x_out, int64_t* ei_out, int64_t ei_stride, int64_t* ea_out,
                   int64_t* batch_out, int64_t num_nodes, int64_t num_edges, int32_t* status,
                   int64_t pad_begin, int64_t pad_end, hipStream_t s) {
  const int64_t mol_blocks = molclr::ceil_div(B, kMolsPerBlock);
  int64_t pad_blocks = molclr::ceil_div(pad_end - pad_begin, 64 * kMolsPerBlock);
  if (pad_blocks > 64) pad_blocks = 64;
  if (mol_blocks + pad_blocks == 0) return;
  hipLaunchKernelGGL(k_task_gather, dim3((unsigned)(mol_blocks + pad_blocks)),
                     dim3(64 * kMolsPerBlock), 0, s, store_x, store_atom_ptr, store_edge_index,
                     store_edge_attr, store_bond_ptr, store_edges, mol_ids, B, store_mols, ptr,
                     edge_off, x_out, ei_out, ei_stride, ea_out, batch_out, num_nodes, num_edges,
                     status, mol_blocks, pad_begin, pad_end);
}

}  // namespace

MOLCLR_API size_t molclr_collate_task_workspace_bytes(int64_t batch_size) {
  if (batch_size < 0) return 0;
  return (size_t)(2 * batch_size + 2) * sizeof(int64_t) + 2 * 256;
}

MOLCLR_API int molclr_collate_task(
    const int64_t* store_x, const int64_t* store_atom_ptr, const int64_t* store_edge_index,
    const int64_t* store_edge_attr, const int64_t* store_bond_ptr, int64_t store_mols,
    int64_t store_edges, const int64_t* mol_ids, int64_t batch_size, const void* target_table,
    int64_t target_cols, int target_is_float, int64_t* x_out, int64_t* edge_index_out,
    int64_t* edge_attr_out, int64_t* batch_out, int64_t* ptr_out, void* target_out,
    int64_t num_nodes, int64_t num_edges, int32_t* status, void* workspace,
    size_t workspace_bytes, molclr_stream_t stream) {
  MOLCLR_TRY_RC(store_args_ok("collate_task", store_x, store_atom_ptr, store_edge_index,
                              store_edge_attr, store_bond_ptr, store_mols, store_edges, mol_ids,
                              batch_size, num_nodes, num_edges));
  MOLCLR_REQUIRE(target_cols >= 1 && (target_is_float || target_cols == 1),
                 "collate_task: targets [rows, %lld] (int64 labels are [rows])",
                 (long long)target_cols);
  MOLCLR_REQUIRE(ptr_out && status && (batch_size == 0 || (target_table && target_out)),
                 "collate_task: null pointer");
  MOLCLR_REQUIRE(num_nodes == 0 || (x_out && batch_out), "collate_task: null pointer");
  MOLCLR_REQUIRE(num_edges == 0 || (edge_index_out && edge_attr_out), "collate_task: null pointer");
  MOLCLR_REQUIRE(aligned16(x_out) && aligned16(edge_attr_out),
                 "collate_task: x_out / edge_attr_out must be 16-byte aligned");
  MOLCLR_REQUIRE_WS(workspace_bytes, molclr_collate_task_workspace_bytes(batch_size));
  MOLCLR_REQUIRE(workspace != nullptr, "collate_task: null workspace");
  hipStream_t s = molclr::as_stream(stream);
  const TaskWs w = task_ws(workspace, workspace_bytes, batch_size);
  TaskOffsets a{store_atom_ptr, store_bond_ptr, mol_ids,     batch_size,  store_mols,
                ptr_out,        w.edge_off,     num_nodes,   num_edges,   status,
                nullptr,        target_table,   target_out,  target_cols, target_is_float};
  hipLaunchKernelGGL(k_task_offsets, dim3(1), dim3(scan_threads(batch_size)), 0, s, a);
  launch_gather(store_x, store_atom_ptr, store_edge_index, store_edge_attr, store_bond_ptr,
                store_mols, store_edges, mol_ids, batch_size, ptr_out, w.edge_off, x_out,
                edge_index_out, num_edges, edge_attr_out, batch_out, num_nodes, num_edges, status,
                0, 0, s);
  MOLCLR_LAUNCHED();
  return MOLCLR_OK;
}

MOLCLR_API int molclr_stage_task_ids(
    const int64_t* store_x, const int64_t* store_atom_ptr, const int64_t* store_edge_index,
    const int64_t* store_edge_attr, const int64_t* store_bond_ptr, int64_t store_mols,
    int64_t store_edges, const int64_t* mol_ids, int64_t batch_size, const void* target_table,
    int64_t target_cols, int target_is_float, int64_t num_nodes, int64_t num_edges,
    const molclr_graph_staged_segment* dst, int64_t* x_all, int64_t num_nodes_cap,
    int64_t num_edges_cap, int64_t* counts, void* target_dst, int32_t* status, void* workspace,
    size_t workspace_bytes, molclr_stream_t stream) {
  MOLCLR_TRY_RC(store_args_ok("stage_task_ids", store_x, store_atom_ptr, store_edge_index,
                              store_edge_attr, store_bond_ptr, store_mols, store_edges, mol_ids,
                              batch_size, num_nodes, num_edges));
  MOLCLR_REQUIRE(target_cols >= 1 && (target_is_float || target_cols == 1),
                 "stage_task_ids: targets [rows, %lld] (int64 labels are [rows])",
                 (long long)target_cols);
  MOLCLR_REQUIRE(status && (batch_size == 0 || (target_table && target_dst)),
                 "stage_task_ids: null pointer");
  MOLCLR_REQUIRE(dst && batch_size == dst[0].num_graphs,
                 "stage_task_ids: %lld molecule ids, the staged graph holds %lld molecules",
                 (long long)batch_size, (long long)(dst ? dst[0].num_graphs : 0));
  // molclr_stage_task's refusals, by its own plan: the store stands in for the
  // source buffers, the jobs are not launched
  molclr::StageJobs jb{};
  int nj = 0;
  int64_t most = 1;
  const molclr_stage_source fake{store_x, store_edge_index, store_edge_attr, store_atom_ptr,
                                 num_nodes, num_edges};
  MOLCLR_TRY_RC(molclr::stage_plan("stage_task_ids", 1, &fake, dst, x_all, num_nodes_cap,
                                   num_edges_cap, counts, jb, nj, most));
  MOLCLR_REQUIRE(aligned16(x_all) && aligned16(dst[0].edge_attr),
                 "stage_task_ids: x_all / edge_attr must be 16-byte aligned");
  MOLCLR_REQUIRE_WS(workspace_bytes, molclr_collate_task_workspace_bytes(batch_size));
  MOLCLR_REQUIRE(workspace != nullptr, "stage_task_ids: null workspace");
  hipStream_t s = molclr::as_stream(stream);
  const TaskWs w = task_ws(workspace, workspace_bytes, batch_size);
  TaskOffsets a{store_atom_ptr, store_bond_ptr, mol_ids,     batch_size,  store_mols,
                w.ptr,          w.edge_off,     num_nodes,   num_edges,   status,
                counts,         target_table,   target_dst,  target_cols, target_is_float};
  hipLaunchKernelGGL(k_task_offsets, dim3(1), dim3(scan_threads(batch_size)), 0, s, a);
  launch_gather(store_x, store_atom_ptr, store_edge_index, store_edge_attr, store_bond_ptr,
                store_mols, store_edges, mol_ids, batch_size, w.ptr, w.edge_off, x_all,
                const_cast<int64_t*>(dst[0].edge_index), dst[0].edge_cap,
                const_cast<int64_t*>(dst[0].edge_attr), const_cast<int64_t*>(dst[0].batch),
                num_nodes, num_edges, status, num_nodes, num_nodes_cap, s);
  MOLCLR_LAUNCHED();
  return MOLCLR_OK;
}

// ---- motif items --------------------------------------------------------------
namespace {
struct MotifWs {
  int64_t* item_off;  // [B + 1]
  int32_t* flags;     // [1]
  int64_t *mol_idx, *clique_idx;  // the staged form's scratch: [T_cap + B], [T_cap]
};
MotifWs motif_ws(void* w, size_t bytes, int64_t B, int64_t T_cap) {
  molclr::Workspace ws(w, bytes);
  MotifWs a;
  a.item_off = ws.take<int64_t>(B + 1);
  a.flags = ws.take<int32_t>(1);
  a.mol_idx = ws.take<int64_t>(T_cap + B);
  a.clique_idx = ws.take<int64_t>(T_cap > 0 ? T_cap : 1);
  return a;
}

int motif_args_ok(const char* who, const int64_t* motif_ptr, const int64_t* motif_ids,
                  int64_t store_mols, const int64_t* mol_ids, int64_t B, int64_t T) {
  if (!(B >= 1 && B < ((int64_t)1 << 31) && T >= 0 && T < ((int64_t)1 << 31) && store_mols >= 0)) {
    molclr::set_error("%s: %lld molecules, %lld items", who, (long long)B, (long long)T);
    return MOLCLR_ERR_ARG;
  }
  if (!(motif_ptr && mol_ids && (T == 0 || motif_ids))) {
    molclr::set_error("%s: null pointer", who);
    return MOLCLR_ERR_ARG;
  }
  return MOLCLR_OK;
}

void launch_items(const int64_t* motif_ptr, const int64_t* motif_ids, int64_t store_mols,
                  const int64_t* mol_ids, int64_t B, int64_t T, int64_t* item_off, int32_t* flags,
                  int64_t* mol_idx, int64_t* clique_idx, int32_t* status, hipStream_t s) {
  hipLaunchKernelGGL(k_motif_offsets, dim3(1), dim3(scan_threads(B)), 0, s, motif_ptr, store_mols,
                     mol_ids, B, T, item_off, flags, status);
  hipLaunchKernelGGL(k_motif_expand, dim3((unsigned)molclr::ceil_div(T + B, kExpandThreads)),
                     dim3(kExpandThreads), 0, s, motif_ptr, motif_ids, mol_ids, B, T,
                     static_cast<const int64_t*>(item_off), static_cast<const int32_t*>(flags),
                     mol_idx, clique_idx);
}
}  // namespace

MOLCLR_API size_t molclr_motif_items_workspace_bytes(int64_t batch_size) {
  if (batch_size < 0) return 0;
  return (size_t)(batch_size + 1) * sizeof(int64_t) + sizeof(int32_t) + 2 * 256;
}

MOLCLR_API int molclr_motif_items(const int64_t* motif_ptr, const int64_t* motif_ids,
                                  int64_t store_mols, const int64_t* mol_ids, int64_t batch_size,
                                  int64_t T, int64_t* mol_idx, int64_t* clique_idx,
                                  int32_t* status, void* workspace, size_t workspace_bytes,
                                  molclr_stream_t stream) {
  MOLCLR_TRY_RC(motif_args_ok("motif_items", motif_ptr, motif_ids, store_mols, mol_ids, batch_size,
                              T));
  MOLCLR_REQUIRE(mol_idx && status && (T == 0 || clique_idx), "motif_items: null pointer");
  MOLCLR_REQUIRE_WS(workspace_bytes, molclr_motif_items_workspace_bytes(batch_size));
  MOLCLR_REQUIRE(workspace != nullptr, "motif_items: null workspace");
  molclr::Workspace ws(workspace, workspace_bytes);
  int64_t* item_off = ws.take<int64_t>(batch_size + 1);
  int32_t* flags = ws.take<int32_t>(1);
  launch_items(motif_ptr, motif_ids, store_mols, mol_ids, batch_size, T, item_off, flags, mol_idx,
               clique_idx, status, molclr::as_stream(stream));
  MOLCLR_LAUNCHED();
  return MOLCLR_OK;
}

MOLCLR_API size_t molclr_stage_motif_ids_workspace_bytes(int64_t batch_size, int64_t T_cap) {
  if (batch_size < 0 || T_cap < 0) return 0;
  return (size_t)(batch_size + 1 + T_cap + batch_size + (T_cap > 0 ? T_cap : 1)) *
             sizeof(int64_t) + sizeof(int32_t) + 4 * 256;
}

MOLCLR_API int molclr_stage_motif_ids(const int64_t* motif_ptr, const int64_t* motif_ids,
                                      int64_t store_mols, const int64_t* mol_ids,
                                      int64_t batch_size, int64_t T, int64_t T_cap,
                                      int64_t* clique, int32_t* mol_ptr, int64_t* sorted_idx,
                                      int64_t* order, int32_t* status, void* workspace,
                                      size_t workspace_bytes, molclr_stream_t stream) {
  MOLCLR_TRY_RC(motif_args_ok("stage_motif_ids", motif_ptr, motif_ids, store_mols, mol_ids,
                              batch_size, T));
  MOLCLR_REQUIRE(T_cap >= 0 && T_cap < ((int64_t)1 << 31), "stage_motif_ids: capacity %lld",
                 (long long)T_cap);
  MOLCLR_REQUIRE_WS(workspace_bytes, molclr_stage_motif_ids_workspace_bytes(batch_size, T_cap));
  MOLCLR_REQUIRE(workspace != nullptr, "stage_motif_ids: null workspace");
  const MotifWs w = motif_ws(workspace, workspace_bytes, batch_size, T_cap);
  // more items than the buffers hold: nothing is expanded, and
  // molclr_stage_motif refuses them as it does its own
  if (T <= T_cap)
    launch_items(motif_ptr, motif_ids, store_mols, mol_ids, batch_size, T, w.item_off, w.flags,
                 w.mol_idx, w.clique_idx, nullptr, molclr::as_stream(stream));
  MOLCLR_LAUNCHED();
  return molclr_stage_motif(w.mol_idx, w.clique_idx, T, batch_size, T_cap, clique, mol_ptr,
                            sorted_idx, order, status, stream);
}
