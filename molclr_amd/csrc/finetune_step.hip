// The captured fine-tuning step's own launches (molclr_amd/finetune_step.py;
// the reference's loops are finetune.py:89-102 for a training batch and
// finetune.py:259-317 for an evaluation pass):
//   molclr_stage_task       outside the graph: the batch and its targets into
//                           the fixed buffers a replay reads (one launch)
//   molclr_stage_motif      outside the graph: the motif model's items into
//                           fixed buffers of an item capacity, with mol_ptr and
//                           the stable sort by motif id the pool's backward
//                           reads (one launch)
//   molclr_task_step_tail   the training graph's closing launch
//   molclr_eval_tail        the evaluation graph's closing launch: gathers
//                           the batch's predictions, targets and loss behind a
//                           device cursor, so a whole pass needs one host copy
// Every copy is a kernel (common.h: captured memset / memcpy nodes).
#include "common.h"
#include "stage.h"

namespace {

__global__ void k_task_step_tail(int32_t* step_a, int32_t* step_b, const float* loss_src,
                                 float* loss_dst, const int32_t* status_src, int32_t* status_acc) {
  if (step_a) *step_a += 1;
  if (step_b) *step_b += 1;
  if (loss_dst) *loss_dst = *loss_src;
  if (status_acc) *status_acc |= *status_src;
}

// one block: every thread reads the cursor before thread 0 advances it
__global__ __launch_bounds__(256) void k_eval_tail(
    const float* __restrict__ pred, const uint32_t* __restrict__ target, int64_t B, int64_t C,
    int64_t tw, const float* __restrict__ loss, float* __restrict__ pred_all,
    uint32_t* __restrict__ target_all, int64_t capacity, int64_t* cursor, double* loss_acc,
    const int32_t* status_src, int32_t* status_acc) {
  const int64_t n = *cursor;
  const bool fits = n >= 0 && n <= capacity - B;
  __syncthreads();
  if (fits) {
    for (int64_t i = threadIdx.x; i < B * C; i += blockDim.x) pred_all[n * C + i] = pred[i];
    for (int64_t i = threadIdx.x; i < B * tw; i += blockDim.x) target_all[n * tw + i] = target[i];
  }
  if (threadIdx.x == 0) {
    int32_t st = status_src ? *status_src : 0;
    if (fits) {
      *loss_acc += (double)*loss * (double)B;  // total += loss.item() * data.y.size(0)
      *cursor = n + B;
    } else {
      st |= MOLCLR_STATUS_EVAL_OVERFLOW;
    }
    if (st) *status_acc |= st;
  }
}

constexpr int kItemThreads = 256;

// A batch's motif items into buffers of capacity T_cap.  Thread i owns staged
// position i: its id v_i is clique_idx[i] or, from T on, the padding value, and
// its place in the stable sort is its rank -- the number of positions j with
// (v_j, j) < (v_i, i) -- counted over LDS tiles of the ids, which every block
// reads from the source itself (no block waits for another).  Block 0 also
// checks mol_idx and writes mol_ptr; T is 0 here when the items were refused.
__global__ __launch_bounds__(kItemThreads) void k_stage_motif(
    const int64_t* __restrict__ mol_idx, const int64_t* __restrict__ clique_idx, int64_t T,
    int64_t rows, int64_t B, int64_t T_cap, int64_t* __restrict__ clique,
    int32_t* __restrict__ mol_ptr, int64_t* __restrict__ sorted_idx, int64_t* __restrict__ order,
    int32_t* status, int32_t refused) {
  __shared__ int64_t s_v[kItemThreads];
  const int64_t i = (int64_t)blockIdx.x * kItemThreads + threadIdx.x;
  const int64_t v = i < T ? clique_idx[i] : MOLCLR_MOTIF_PAD;
  int64_t rank = 0;
  for (int64_t j0 = 0; j0 < T_cap; j0 += kItemThreads) {
    const int64_t j = j0 + threadIdx.x;
    s_v[threadIdx.x] = j < T ? clique_idx[j] : MOLCLR_MOTIF_PAD;
    __syncthreads();
    const int n = (int)(T_cap - j0 < kItemThreads ? T_cap - j0 : kItemThreads);
    for (int q = 0; q < n; ++q) {
      const int64_t u = s_v[q];
      rank += (u < v || (u == v && j0 + q < i)) ? 1 : 0;
    }
    __syncthreads();
  }
  if (i < T_cap) {  // rank is a permutation of [0, T_cap)
    clique[i] = v;
    sorted_idx[rank] = v;
    order[rank] = i;
  }
  if (blockIdx.x != 0) return;
  // mol_idx: [rows] values in [0, B), the first T of them ascending
  __shared__ int32_t s_bits;
  if (threadIdx.x == 0) s_bits = refused;
  __syncthreads();
  int32_t mine = 0;
  for (int64_t k = threadIdx.x; k < rows; k += kItemThreads) {
    const int64_t m = mol_idx[k];
    if (m < 0 || m >= B) mine |= MOLCLR_STATUS_ITEM_MOL;
    if (k > 0 && k < T && mol_idx[k - 1] > m) mine |= MOLCLR_STATUS_ITEM_ORDER;
  }
  if (mine) atomicOr(&s_bits, mine);
  __syncthreads();
  const int32_t bits = s_bits;
  if (bits && threadIdx.x == 0 && status) atomicOr(status, bits);
  for (int64_t b = threadIdx.x; b <= B; b += kItemThreads) {
    int64_t lo = 0, hi = T;  // first item of a molecule >= b
    while (lo < hi) {
      const int64_t mid = lo + (hi - lo) / 2;
      if (mol_idx[mid] < b) lo = mid + 1; else hi = mid;
    }
    // refused items: a pointer the pool flags, so no molecule's row is trusted
    mol_ptr[b] = bits ? -1 : (int32_t)lo;
  }
}

}  // namespace

MOLCLR_API int molclr_stage_motif(const int64_t* mol_idx, const int64_t* clique_idx, int64_t T,
                                  int64_t B, int64_t T_cap, int64_t* clique, int32_t* mol_ptr,
                                  int64_t* sorted_idx, int64_t* order, int32_t* status,
                                  molclr_stream_t stream) {
  MOLCLR_REQUIRE(B >= 1 && B < ((int64_t)1 << 31) && T >= 0 && T_cap >= 0 &&
                     T_cap < ((int64_t)1 << 31),
                 "stage_motif: %lld molecules, %lld items, capacity %lld", (long long)B,
                 (long long)T, (long long)T_cap);
  MOLCLR_REQUIRE(mol_idx && mol_ptr && (T == 0 || clique_idx) &&
                     (T_cap == 0 || (clique && sorted_idx && order)),
                 "stage_motif: null pointer");
  // more items than the buffers hold: nothing of them is staged
  const bool over = T > T_cap;
  int64_t blocks = molclr::ceil_div(T_cap, kItemThreads);
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_stage_motif, dim3((unsigned)blocks), dim3(kItemThreads), 0,
                     molclr::as_stream(stream), mol_idx, clique_idx, over ? 0 : T,
                     over ? 0 : T + B, B, T_cap, clique, mol_ptr, sorted_idx, order, status,
                     over ? MOLCLR_STATUS_ITEM_OVERFLOW : 0);
  MOLCLR_LAUNCHED();
  return MOLCLR_OK;
}

MOLCLR_API int molclr_stage_task(const molclr_stage_source* src,
                                 const molclr_graph_staged_segment* dst, int64_t* x_all,
                                 int64_t num_nodes_cap, int64_t num_edges_cap, int64_t* counts,
                                 const void* target_src, void* target_dst, int64_t target_rows,
                                 int64_t target_cols, int target_is_float,
                                 molclr_stream_t stream) {
  MOLCLR_REQUIRE(target_rows >= 0 && target_cols >= 1 && (target_is_float || target_cols == 1),
                 "stage_task: targets [%lld, %lld] (int64 labels are [rows])",
                 (long long)target_rows, (long long)target_cols);
  const int64_t nwords = target_is_float ? target_rows * target_cols : 2 * target_rows;
  MOLCLR_REQUIRE(nwords == 0 || (target_src && target_dst), "stage_task: null target buffer");
  MOLCLR_REQUIRE(dst && target_rows == dst[0].num_graphs,
                 "stage_task: %lld target rows, the staged graph holds %lld molecules",
                 (long long)target_rows, (long long)(dst ? dst[0].num_graphs : 0));
  molclr::StageJobs jb{};
  int nj = 0;
  int64_t most = 1;
  MOLCLR_TRY_RC(molclr::stage_plan("stage_task", 1, src, dst, x_all, num_nodes_cap, num_edges_cap,
                                   counts, jb, nj, most));
  jb.words_src = static_cast<const uint32_t*>(target_src);
  jb.words_dst = static_cast<uint32_t*>(target_dst);
  jb.nwords = nwords;
  if (nwords > most) most = nwords;
  molclr::stage_launch(jb, nj, most, molclr::as_stream(stream));
  MOLCLR_LAUNCHED();
  return MOLCLR_OK;
}

MOLCLR_API int molclr_task_step_tail(int32_t* step_a, int32_t* step_b, const float* loss_src,
                                     float* loss_dst, const int32_t* status_src,
                                     int32_t* status_acc, molclr_stream_t stream) {
  MOLCLR_REQUIRE((!loss_dst || loss_src) && (!status_acc || status_src),
                 "task_step_tail: null pointer");
  hipLaunchKernelGGL(k_task_step_tail, dim3(1), dim3(1), 0, molclr::as_stream(stream), step_a,
                     step_b, loss_src, loss_dst, status_src, status_acc);
  MOLCLR_LAUNCHED();
  return MOLCLR_OK;
}

MOLCLR_API int molclr_eval_tail(const float* pred, const void* target, int64_t B, int64_t C,
                                int64_t target_row_words, const float* loss, float* pred_all,
                                void* target_all, int64_t capacity, int64_t* cursor,
                                double* loss_acc, const int32_t* status_src, int32_t* status_acc,
                                molclr_stream_t stream) {
  MOLCLR_REQUIRE(B >= 1 && C >= 1 && target_row_words >= 1 && capacity >= 0,
                 "eval_tail: B %lld, C %lld, %lld target words per row, capacity %lld",
                 (long long)B, (long long)C, (long long)target_row_words, (long long)capacity);
  MOLCLR_REQUIRE(pred && target && loss && pred_all && target_all && cursor && loss_acc &&
                     status_acc,
                 "eval_tail: null pointer");
  hipLaunchKernelGGL(k_eval_tail, dim3(1), dim3(256), 0, molclr::as_stream(stream), pred,
                     static_cast<const uint32_t*>(target), B, C, target_row_words, loss, pred_all,
                     static_cast<uint32_t*>(target_all), capacity, cursor, loss_acc, status_src,
                     status_acc);
  MOLCLR_LAUNCHED();
  return MOLCLR_OK;
}
