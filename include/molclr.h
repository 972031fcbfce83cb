/*
 * molclr.h — C ABI of the MI355X-native MolCLR pre-training hot path.
 *
 * This is the drop-in boundary: every entry point is `extern "C"`, takes plain
 * device pointers, element counts and an opaque HIP stream (`void*`, a
 * `hipStream_t`), and returns 0 on success or a non-zero status
 * (MOLCLR_ERR_* below, or a positive hipError_t).  `molclr_last_error()` gives
 * a thread-local message for the last failure.  No entry point allocates,
 * synchronises the device, or keeps state between calls: the caller owns
 * every buffer (including the `workspace` scratch, sized by the matching
 * `*_workspace_bytes` query) and all work is stream-ordered, so a caller may
 * capture any sequence of these calls into a HIP graph.
 *
 * Reference interfaces replaced (CameronDiao/MolCLR @ /root/reference):
 *   - PyG 1.6.3 `add_self_loops` + self-loop edge attr, done per layer in
 *       models/ginet_molclr.py:31-37 and models/gcn_molclr.py:64-70
 *       -> molclr_graph_build (once per batch, self loops implicit)
 *   - MoleculeDataset.__getitem__ node-mask views (dataset/dataset.py:111-145)
 *       + the DataLoader's PyG collate    -> molclr_mask_views (on device)
 *   - atom embedding   models/ginet_molclr.py:103, models/gcn_molclr.py:144
 *       -> molclr_atom_embed_fwd / _bwd
 *   - GINEConv edge embedding + message + PyG aggr='add'
 *       models/ginet_molclr.py:39-44        -> molclr_gine_aggregate_fwd / _bwd
 *   - GCNConv message + aggr='add' + bias
 *       models/gcn_molclr.py:72-88          -> molclr_gcn_aggregate_fwd / _bwd (and _bf16)
 *   - nn.Linear (GIN MLP ginet_molclr.py:19-23, heads :90-96), GCN `x @ W`
 *       (gcn_molclr.py:76) and their autograd -> molclr_gemm_f32, molclr_colsum_f32
 *   - BatchNorm1d(train/eval) + ReLU + dropout(p=0)
 *       models/ginet_molclr.py:107-111     -> molclr_batchnorm_fwd / _bwd
 *   - global_mean_pool / global_add_pool  ginet_molclr.py:113
 *                                           -> molclr_segment_pool_fwd / _bwd
 *   - F.normalize(dim=1)                  molclr.py:63-64 -> molclr_l2norm_fwd / _bwd
 *   - NTXentLoss.forward (cosine / dot)   utils/nt_xent.py:33-65
 *                                           -> molclr_ntxent_fwd / _bwd
 *   - torch.optim.Adam(weight_decay=L2)   molclr.py:84-87,127 -> molclr_adam_step
 */
#ifndef MOLCLR_H_
#define MOLCLR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* molclr_stream_t; /* a hipStream_t; NULL = legacy default stream */

enum {
  MOLCLR_OK = 0,
  MOLCLR_ERR_ARG = -1,       /* bad shape / pointer / size argument */
  MOLCLR_ERR_WORKSPACE = -2, /* workspace too small */
  MOLCLR_ERR_UNSUPPORTED = -3
};

/* Vocabulary of the reference (models/ginet_molclr.py:9-13). */
#define MOLCLR_NUM_ATOM_TYPE 119     /* 118 elements + mask token 118 */
#define MOLCLR_NUM_CHIRALITY 3
#define MOLCLR_NUM_BOND_TYPE 5       /* 4 bond types + self-loop type 4 */
#define MOLCLR_NUM_BOND_DIR 3
#define MOLCLR_SELF_LOOP_BOND_TYPE 4 /* ginet_molclr.py:35 */
#define MOLCLR_ECOUNT_STRIDE 8       /* per-node counts: 5 bond types, 3 dirs */
#define MOLCLR_NUM_ECOMB 15          /* combined edge-table rows: bt * 3 + bd */
#define MOLCLR_SELF_LOOP_ECOMB 12    /* bond type 4, dir 0 */
#define MOLCLR_NBR_SLOTS 4           /* in-edges held in a node's neighbour slots */
#define MOLCLR_NBR_OVERFLOW 7        /* degree field: > MOLCLR_NBR_SLOTS, use the CSR */
#define MOLCLR_NBR_MAX_NODES (1 << 24)
/* bit of a graph's status word (molclr_graph_build) that the atom embedding
 * sets when an atom type or chirality index lies outside its table */
#define MOLCLR_STATUS_ATOM_RANGE 8

/* ecode (bond_type | bond_dir << 3) -> combined edge-table row */
#define MOLCLR_ECOMB(ecode) ((int)((ecode) & 7u) * 3 + (int)((ecode) >> 3))

const char* molclr_version(void);
const char* molclr_last_error(void);

/* ------------------------------------------------------------------------
 * Graph build (once per batch and view).
 * Inputs are the PyG Batch fields exactly as the reference collates them
 * (dataset/dataset.py:86-147 + PyG collate): edge_index int64 [2,E]
 * (row 0 = source j, row 1 = destination i, flow source_to_target),
 * edge_attr int64 [E,2] (bond type 0..4, bond dir 0..2), batch int64 [N]
 * (ascending, graphs contiguous).
 * Outputs (device, caller-allocated):
 *   rowptr [N+1] i32, col [E] i32, ecode [E] u8 : in-edges of every node
 *       sorted stably by destination (edge order kept inside a row) — the
 *       order in which PyG's scatter-add accumulates them; the self loop PyG
 *       appends at the end of the edge list is implicit (applied last).
 *       ecode = bond_type | bond_dir << 3.
 *   rowptr_t [N+1] i32, col_t [E] i32 : out-edges sorted stably by source
 *       (the accumulation order of index_select's backward).
 *   nbr [N*4] u32, nbr_t [N*4] u32 : neighbour slots, one 16-byte entry per
 *       node so the aggregation reads a row's neighbours with one load and
 *       no rowptr -> col dependency.  Entry i holds the first 4 CSR (nbr) /
 *       CSC (nbr_t) neighbours of i in row order; nbr packs
 *       src | MOLCLR_ECOMB(ecode) << 24.  Bits 29..31 of word 0 hold the
 *       degree, or MOLCLR_NBR_OVERFLOW when it exceeds 4 (the kernels then
 *       walk the CSR/CSC row instead).  Requires N <= MOLCLR_NBR_MAX_NODES.
 *   ecount [N*8] i32 : per destination, counts of in-edge bond types 0..4
 *       and bond dirs 0..2, self loop included.
 *   graph_ptr [G+1] i32 : node range of every graph.
 *   status [1] i32 : bit 0 edge index out of range, bit 1 edge attr out of
 *       range, bit 2 batch not ascending / out of range.  Offending entries
 *       are clamped so no later kernel reads out of bounds.  The encoders'
 *       atom embedding adds bit 3 (MOLCLR_STATUS_ATOM_RANGE) when handed the
 *       word.
 * ------------------------------------------------------------------------ */
size_t molclr_graph_build_workspace_bytes(int64_t num_nodes, int64_t num_edges);
int molclr_graph_build(const int64_t* edge_index, const int64_t* edge_attr,
                       const int64_t* batch, int64_t num_nodes, int64_t num_edges,
                       int64_t num_graphs, int32_t* rowptr, int32_t* col,
                       uint8_t* ecode, int32_t* rowptr_t, int32_t* col_t,
                       uint32_t* nbr, uint32_t* nbr_t,
                       int32_t* ecount, int32_t* graph_ptr, int32_t* status,
                       void* workspace, size_t workspace_bytes, molclr_stream_t stream);

/* molclr_graph_build over `nseg` (<= MOLCLR_MAX_SEGMENTS) PyG batches taken as
 * one: segment s's nodes / edges / graphs follow those of segments 0..s-1
 * (edge_index values stay local to their segment).  The two contrastive
 * views of a step are built as ONE graph this way and run through one
 * encoder pass (molclr_batchnorm_seg_fwd keeps their statistics apart).
 * Workspace: molclr_graph_build_workspace_bytes(total nodes, total edges). */
#define MOLCLR_MAX_SEGMENTS 8
typedef struct molclr_graph_segment {
  const int64_t* edge_index; /* [2, num_edges] */
  const int64_t* edge_attr;  /* [num_edges, 2] */
  const int64_t* batch;      /* [num_nodes] */
  int64_t num_nodes, num_edges, num_graphs;
} molclr_graph_segment;
int molclr_graph_build_multi(int nseg, const molclr_graph_segment* segs, int32_t* rowptr,
                             int32_t* col, uint8_t* ecode, int32_t* rowptr_t, int32_t* col_t,
                             uint32_t* nbr, uint32_t* nbr_t, int32_t* ecount, int32_t* graph_ptr,
                             int32_t* status, void* workspace, size_t workspace_bytes,
                             molclr_stream_t stream);

/* Device-sized graph build: molclr_graph_build_multi over fixed-capacity
 * buffers, for a training step captured once as a HIP graph and replayed for
 * every batch that fits (molclr_amd/graph_step.py; the reference's per-step
 * loop, molclr.py:107-128).  Two calls:
 *   molclr_stage_segments (outside the captured region; one launch): copies
 *     segment s's PyG fields -- x [n_s,2], edge_index [2,e_s], edge_attr
 *     [e_s,2], batch [n_s] -- into its staging buffers dst[s] (edge_index
 *     rows edge_cap apart), x into x_all [num_nodes_cap,2] at row
 *     n_0 + .. + n_{s-1}, fills the remaining rows of x_all with atom (0, 0),
 *     and writes counts [2*nseg] = n_0..n_{nseg-1}, e_0..e_{nseg-1}.
 *   molclr_graph_build_dev (inside it): the build, reading the counts on the
 *     device.  Outputs sized for num_nodes_cap rows / num_edges_cap edges
 *     (workspace: molclr_graph_build_workspace_bytes of those); rows past the
 *     real nodes are padding: no edges, ecount = the self loop only, outside
 *     every graph (graph_ptr[G] = the real node count).  G = sum of num_graphs
 *     is fixed. */
typedef struct molclr_stage_source {
  const int64_t *x, *edge_index, *edge_attr, *batch;
  int64_t num_nodes, num_edges;
} molclr_stage_source;
typedef struct molclr_graph_staged_segment {
  const int64_t* edge_index; /* [2, edge_cap] */
  const int64_t* edge_attr;  /* [edge_cap, 2] */
  const int64_t* batch;      /* [node_cap] */
  int64_t node_cap, edge_cap, num_graphs;
} molclr_graph_staged_segment;
int molclr_stage_segments(int nseg, const molclr_stage_source* src,
                          const molclr_graph_staged_segment* dst, int64_t* x_all,
                          int64_t num_nodes_cap, int64_t num_edges_cap, int64_t* counts,
                          molclr_stream_t stream);
int molclr_graph_build_dev(int nseg, const molclr_graph_staged_segment* segs, const int64_t* counts,
                           int64_t num_nodes_cap, int64_t num_edges_cap, int32_t* rowptr,
                           int32_t* col, uint8_t* ecode, int32_t* rowptr_t, int32_t* col_t,
                           uint32_t* nbr, uint32_t* nbr_t, int32_t* ecount, int32_t* graph_ptr,
                           int32_t* status, void* workspace, size_t workspace_bytes,
                           molclr_stream_t stream);

/* On-device node-mask augmentation + collate: one contrastive view of a batch
 * of molecules, replacing MoleculeDataset.__getitem__'s masking
 * (dataset/dataset.py:111-145) and the DataLoader's PyG collate
 * (Batch.from_data_list).  Per molecule: max(1, floor(N/4)) atoms become
 * [118, 0]; floor(M/4) bonds are dropped with both directed edges; the kept
 * edges stay in store order.  The subsets are uniform, drawn from splitmix64
 * keys of (seed, view, molecule id, item) (restated in oracle/augment_ref.py).
 * Store (device, int64): x [Ntot,2]; atom_ptr [G+1]; edge_index [2,store_edges]
 * with molecule-local atom indices, molecule g's bonds as the directed pairs
 * 2b, 2b+1 for b in [bond_ptr[g], bond_ptr[g+1]); edge_attr [store_edges,2].
 * mol_ids [batch_size] picks the batch.  Outputs (caller-sized: num_nodes =
 * Σ N_g, num_edges = Σ 2 (M_g - floor(M_g/4))): x_out [num_nodes,2],
 * edge_index_out [2,num_edges], edge_attr_out [num_edges,2], batch_out
 * [num_nodes], ptr_out [batch_size+1] -- the Batch fields.  status [1] i32:
 * bit 0 molecule id out of range, bit 1 output sizes do not match the batch,
 * bit 2 store edge index out of its molecule's range (clamped).  view: 0 / 1. */
size_t molclr_mask_views_workspace_bytes(int64_t batch_size);
int molclr_mask_views(const int64_t* store_x, const int64_t* store_atom_ptr,
                      const int64_t* store_edge_index, const int64_t* store_edge_attr,
                      const int64_t* store_bond_ptr, int64_t store_mols, int64_t store_edges,
                      const int64_t* mol_ids, int64_t batch_size, uint64_t seed, int view,
                      int64_t* x_out, int64_t* edge_index_out, int64_t* edge_attr_out,
                      int64_t* batch_out, int64_t* ptr_out, int64_t num_nodes, int64_t num_edges,
                      int32_t* status, void* workspace, size_t workspace_bytes,
                      molclr_stream_t stream);

/* On-device subgraph-removal views (dataset/dataset_subgraph.py:70-177,
 * mode MOLCLR_AUG_SUBGRAPH) and mixed subgraph + atom/bond masking views
 * (dataset/dataset_mix.py:46-217, mode MOLCLR_AUG_MIX) + collate, from the
 * molclr_mask_views store.  Per molecule: the networkx BFS removal
 * (removeSubgraph: from a random centre, floor(p x atoms-in-bonds) atoms,
 * p = 0.25 or uniform [0, 0.2) in mix, the frontier in CPython set order)
 * masks the removed atoms to [118, 0]; bonds survive as G_i.edges keeps them
 * (mix: both atoms remain; subgraph: additionally (start, end) must be
 * networkx's orientation); mix then masks max(0, floor(N/4) - removed) more
 * atoms among the remaining and drops max(0, kept - ceil(3M/4)) surviving
 * bonds.  Two calls because the edge count is data dependent:
 *   plan: ptr_out [B+1] (atom offsets), *num_edges_out (device int64) =
 *         the view's directed-edge count; the plan lives in the workspace;
 *   write: the Batch fields (as molclr_mask_views) sized by that count.
 * num_nodes = Σ atoms, num_bonds = Σ bonds of the batch's molecules.  status
 * bits: 0 molecule id out of range, 1 num_nodes mismatch, 2 edge index out
 * of its molecule (clamped), 3 the frontier emptied before the quota (the
 * subgraph module would not terminate; dataset_mix.py:55-56's guard is
 * applied), 4 a molecule over 256 atoms / 512 bonds (left un-augmented; with
 * molclr_aug_views_plan_big: over its large-molecule caps), 5 a centre atom
 * without bonds (the reference raises). */
enum { MOLCLR_AUG_SUBGRAPH = 0, MOLCLR_AUG_MIX = 1 };
size_t molclr_aug_views_workspace_bytes(int64_t batch_size, int64_t num_nodes, int64_t num_bonds);
int molclr_aug_views_plan(const int64_t* store_atom_ptr, const int64_t* store_edge_index,
                          const int64_t* store_bond_ptr, int64_t store_mols, int64_t store_edges,
                          const int64_t* mol_ids, int64_t batch_size, uint64_t seed, int view,
                          int mode, int64_t num_nodes, int64_t num_bonds, int64_t* ptr_out,
                          int64_t* num_edges_out, int32_t* status, void* workspace,
                          size_t workspace_bytes, molclr_stream_t stream);
/* The plan with molecules beyond the in-LDS caps (256 atoms / 512 bonds)
 * augmented too, the reference's behaviour for every molecule
 * (dataset_subgraph.py:96-177 and dataset_mix.py:86-217 have no size limit):
 * they run the same plan over int32 tables in `big_workspace`, one slot per
 * such molecule of the batch.  big_slots >= the batch's count of such
 * molecules, big_atoms / big_bonds >= their largest atom / bond counts
 * (molecules past these caps pass unchanged, status bit 4).  Results are
 * identical to molclr_aug_views_plan's on every molecule within its caps. */
size_t molclr_aug_views_big_workspace_bytes(int64_t big_slots, int64_t big_atoms,
                                            int64_t big_bonds);
int molclr_aug_views_plan_big(const int64_t* store_atom_ptr, const int64_t* store_edge_index,
                              const int64_t* store_bond_ptr, int64_t store_mols,
                              int64_t store_edges, const int64_t* mol_ids, int64_t batch_size,
                              uint64_t seed, int view, int mode, int64_t num_nodes,
                              int64_t num_bonds, int64_t* ptr_out, int64_t* num_edges_out,
                              int32_t* status, void* workspace, size_t workspace_bytes,
                              int64_t big_slots, int64_t big_atoms, int64_t big_bonds,
                              void* big_workspace, size_t big_workspace_bytes,
                              molclr_stream_t stream);
int molclr_aug_views_write(const int64_t* store_x, const int64_t* store_atom_ptr,
                           const int64_t* store_edge_index, const int64_t* store_edge_attr,
                           const int64_t* store_bond_ptr, int64_t store_mols, int64_t store_edges,
                           const int64_t* mol_ids, int64_t batch_size, const int64_t* ptr,
                           int64_t num_nodes, int64_t num_bonds, int64_t num_edges, int64_t* x_out,
                           int64_t* edge_index_out, int64_t* edge_attr_out, int64_t* batch_out,
                           const void* workspace, size_t workspace_bytes, molclr_stream_t stream);

/* Atom embedding: h[i] = X1[x[i,0]] + X2[x[i,1]]  (ginet_molclr.py:103).
 * x int64 [N,2]; X1 [n1,D], X2 [n2,D]; h [N,D] f32.  A node whose atom type
 * or chirality lies outside [0,n1) / [0,n2) -- where the reference's
 * nn.Embedding raises -- gets a NaN row and sets MOLCLR_STATUS_ATOM_RANGE in
 * *status (nullable: e.g. the batch's graph status word). */
int molclr_atom_embed_fwd(const int64_t* x, const float* X1, const float* X2,
                          float* h, int64_t num_nodes, int64_t dim, int64_t n1,
                          int64_t n2, int32_t* status, molclr_stream_t stream);
/* dX1 [n1,D], dX2 [n2,D] = Σ over nodes of each type of dh (deterministic, fp64
 * accumulation).  accumulate != 0 adds into dX1/dX2 (fused gradient
 * accumulation into a parameter's .grad); the same flag on the other
 * backward entry points below applies to their parameter-gradient outputs. */
size_t molclr_atom_embed_bwd_workspace_bytes(int64_t num_nodes, int64_t dim, int64_t n1,
                                             int64_t n2);
int molclr_atom_embed_bwd(const int64_t* x, const float* dh, float* dX1, float* dX2,
                          int64_t num_nodes, int64_t dim, int64_t n1, int64_t n2, int accumulate,
                          void* workspace, size_t workspace_bytes, molclr_stream_t stream);

/* Combined edge tables of `layers` GINE layers (ginet_molclr.py:24-27,39):
 *   Ec[l][bt*3 + bd][:] = E1_l[bt][:] + E2_l[bd][:]
 * (the edge embedding the reference computes per edge, one fp32 rounding —
 * so using Ec is bit-identical).  E1s / E2s are HOST arrays of `layers`
 * device pointers to [5,D] / [3,D] tables; Ec is [layers, 15, D].
 * layers <= MOLCLR_MAX_LAYERS.  One launch for all layers. */
#define MOLCLR_MAX_LAYERS 16
int molclr_edge_tables_combine(int layers, const float* const* E1s, const float* const* E2s,
                               float* Ec, int64_t dim, molclr_stream_t stream);

/* GINE aggregation (ginet_molclr.py:39-44 + PyG aggr='add'):
 *   out[i] = Σ_{k in in(i), edge order} (x[src_k] + Ec[bt_k*3+bd_k])
 *            + (x[i] + Ec[12])                              (self loop last)
 * Same operation order as the reference CPU path, so results are
 * bit-identical to it.  x, out [N,D] f32; Ec [15,D] (molclr_edge_tables_combine);
 * nbr from molclr_graph_build, with rowptr/col/ecode for rows of degree > 4. */
int molclr_gine_aggregate_fwd(const float* x, const int32_t* rowptr, const int32_t* col,
                              const uint8_t* ecode, const uint32_t* nbr, const float* Ec,
                              float* out, int64_t num_nodes, int64_t dim,
                              molclr_stream_t stream);
/* molclr_gine_aggregate_fwd that also writes the output's row maxima and,
 * when `slot` is not NULL, folds max |out| into it (zeroed by the caller):
 * the row scales of the h3 product that consumes it (molclr_gemm_f32_h3 with
 * a_row_parts = molclr_rowmax_layout(D)), with no pass of its own.  Layout
 * (molclr_rowmax_layout(D), molclr_rowmax_bytes(N, D) bytes): P > 0: P
 * partial arrays rowparts[p][N] (the row max is the max over p); < 0 (D / 4
 * >= 64): one float2 per 64 float4s of the row-major output (the maxima of
 * the pieces of the wave's first row and of the next row). */
int64_t molclr_rowmax_layout(int64_t D);
size_t molclr_rowmax_bytes(int64_t N, int64_t D);
int molclr_gine_aggregate_fwd_rowmax(const float* x, const int32_t* rowptr, const int32_t* col,
                                     const uint8_t* ecode, const uint32_t* nbr, const float* Ec,
                                     float* out, int64_t N, int64_t D, float* rowparts,
                                     float* slot, molclr_stream_t stream);
/* GINE aggregation whose source is a BatchNorm output that is never stored:
 * z [N,D] is the BatchNorm INPUT and coeffs its apply coefficients (scale
 * [nseg,D], then shift [nseg,D]; molclr_batchnorm_seg_coeffs; 16-byte
 * aligned).  Every source element, the self row's and the gathered rows', is
 * read as y = fma(z, scale, shift), then max(y, 0) when relu -- the
 * arithmetic of molclr_batchnorm_seg_fwd's apply (bf16: y rounded to bf16 as
 * the apply stores it) -- so out is bit-identical to molclr_batchnorm_seg_fwd
 * followed by molclr_gine_aggregate_fwd[_rowmax | _bf16] on its y, without
 * the write of y and its re-read.  Segments as the BatchNorm's: seg_rows
 * (host, summing to N) or, when not NULL, seg_rows_dev (device; N is then the
 * row capacity and rows past the segments' sum are padding whose source reads
 * as zero, the y the apply writes there).
 * PRECONDITION: every in-edge of a row comes from a row of the same segment
 * (true of a batched graph: edges stay inside one molecule); a row's sources
 * take the coefficients of the row's own segment.
 * rowparts (may be NULL) / slot (NULL without rowparts) as
 * molclr_gine_aggregate_fwd_rowmax. */
int molclr_gine_aggregate_bn_fwd(const float* z, const float* coeffs, int relu, int nseg,
                                 const int64_t* seg_rows, const int64_t* seg_rows_dev,
                                 const int32_t* rowptr, const int32_t* col, const uint8_t* ecode,
                                 const uint32_t* nbr, const float* Ec, float* out, int64_t N,
                                 int64_t D, float* rowparts, float* slot, molclr_stream_t stream);
/* Backward: dx[j] = Σ_{k in out(j), edge order} g[dst_k] + g[j];
 * dE1[t] = Σ_i ecount[i][t] g[i], dE2[d] = Σ_i ecount[i][5+d] g[i].
 * dx may be NULL (first layer input needs no grad); dE1/dE2 may be NULL.
 * dim must be a multiple of 4 in [4, 4096] (the edge-table reduction plans its
 * blocks as molclr_colsum_f32 does): any other width is MOLCLR_ERR_ARG, and
 * the workspace query returns 0 for it. */
size_t molclr_gine_aggregate_bwd_workspace_bytes(int64_t num_nodes, int64_t dim);
int molclr_gine_aggregate_bwd(const float* g, const int32_t* rowptr_t, const int32_t* col_t,
                              const uint32_t* nbr_t, const int32_t* ecount, float* dx, float* dE1, float* dE2,
                              int64_t num_nodes, int64_t dim, int accumulate, void* workspace,
                              size_t workspace_bytes, molclr_stream_t stream);
/* molclr_gine_aggregate_bwd with the kernels chosen per call (tests and
 * benchmarks): 0 = the transposed gather, then the edge-table partials (two
 * passes over g); 1 = both in one pass over g when dx and a table gradient are
 * asked for and num_nodes > 0 (otherwise as 0); -1 = automatic, as the call
 * above: 1 unless the environment has MOLCLR_AGG_BWD_FUSED=0 (read once).
 * The results of 0 and 1 are bit-identical. */
int molclr_gine_aggregate_bwd_impl(const float* g, const int32_t* rowptr_t, const int32_t* col_t,
                                   const uint32_t* nbr_t, const int32_t* ecount, float* dx,
                                   float* dE1, float* dE2, int64_t num_nodes, int64_t dim,
                                   int accumulate, void* workspace, size_t workspace_bytes,
                                   molclr_stream_t stream, int impl);

/* GCN aggregation (gcn_molclr.py:72-88; gcn_norm at :74 is computed and
 * discarded by the reference, so it is not computed here):
 *   out[i] = Σ_{k in in(i)} (e_k + xw[src_k]) + (e_self + xw[i]) + bias
 * with scalar e = E1[bt][0] + E2[bd][0] (tables [5,1], [3,1]). */
int molclr_gcn_aggregate_fwd(const float* xw, const int32_t* rowptr, const int32_t* col,
                             const uint8_t* ecode, const uint32_t* nbr, const float* E1,
                             const float* E2,
                             const float* bias, float* out, int64_t num_nodes,
                             int64_t dim, molclr_stream_t stream);
/* Backward: dxw[j] = Σ_{out(j)} g[dst] + g[j]; dE1[t] = Σ_i ecount[i][t]·Σ_d g[i][d];
 * dE2 likewise; dbias = Σ_i g[i].  Any output pointer may be NULL. */
size_t molclr_gcn_aggregate_bwd_workspace_bytes(int64_t num_nodes, int64_t dim);
int molclr_gcn_aggregate_bwd(const float* g, const int32_t* rowptr_t, const int32_t* col_t,
                             const uint32_t* nbr_t, const int32_t* ecount, float* dxw, float* dE1, float* dE2,
                             float* dbias, int64_t num_nodes, int64_t dim, int accumulate,
                             void* workspace, size_t workspace_bytes, molclr_stream_t stream);
/* The same over bf16 storage (see "bf16 storage" below): xw / out and g / dxw
 * are bf16, the tables, the bias and their gradients fp32.  Per element the
 * forward does the fp32 kernel's additions in its order and rounds once, to
 * nearest even, at the store (dim % 8 == 0: 16-byte units; else 8-byte units).
 * The backward's dxw is molclr_gine_aggregate_bwd_bf16's transposed gather;
 * dE1 / dE2 / dbias are summed in fp32 / fp64 by the fp32 entry point's kernels
 * with its partitioning and order, so on the same values they equal its
 * outputs bit for bit.  workspace: molclr_gcn_aggregate_bwd_workspace_bytes. */
int molclr_gcn_aggregate_fwd_bf16(const uint16_t* xw, const int32_t* rowptr, const int32_t* col,
                                  const uint8_t* ecode, const uint32_t* nbr, const float* E1,
                                  const float* E2, const float* bias, uint16_t* out,
                                  int64_t num_nodes, int64_t dim, molclr_stream_t stream);
int molclr_gcn_aggregate_bwd_bf16(const uint16_t* g, const int32_t* rowptr_t,
                                  const int32_t* col_t, const uint32_t* nbr_t,
                                  const int32_t* ecount, uint16_t* dxw, float* dE1, float* dE2,
                                  float* dbias, int64_t num_nodes, int64_t dim, int accumulate,
                                  void* workspace, size_t workspace_bytes,
                                  molclr_stream_t stream);

/* ------------------------------------------------------------------------
 * FP32 GEMM on the gfx950 f32 MFMA (v_mfma_f32_32x32x2_f32: exact f32 FMA
 * chains, no TF32-style truncation).
 *   C[m,n] = Σ_k A(m,k) B(k,n)  (+ epilogue)
 *   A(m,k) = a_kmajor ? A[k*lda + m] : A[m*lda + k]
 *   B(k,n) = b_kmajor ? B[k*ldb + n] : B[n*ldb + k]
 * so nn.Linear forward (x W^T) is a_kmajor=0, b_kmajor=0; dX = dY W is
 * a_kmajor=0, b_kmajor=1; dW = dY^T X is a_kmajor=1, b_kmajor=1.
 * Epilogues: MOLCLR_EPI_NONE, _BIAS (C += bias[n]), _BIAS_RELU,
 * _RELU_MASK (C *= (aux[m*ldaux+n] > 0), the ReLU backward), optionally
 * OR-ed with MOLCLR_EPI_ACCUMULATE (C = C_old + result).
 * An operand stored with K contiguous needs K and its ld to be multiples of 4.
 * Split-K (for the weight-gradient shape, K = number of nodes) runs when the
 * workspace is large enough: molclr_gemm_f32_workspace_bytes(M,N,K). */
enum { MOLCLR_EPI_NONE = 0, MOLCLR_EPI_BIAS = 1, MOLCLR_EPI_BIAS_RELU = 2,
       MOLCLR_EPI_RELU_MASK = 3,
       MOLCLR_EPI_ACCUMULATE = 16 /* OR-able flag: C += result (gradient accumulation) */ };
size_t molclr_gemm_f32_workspace_bytes(int64_t M, int64_t N, int64_t K);
int molclr_gemm_f32(const float* A, const float* B, float* C, int64_t M, int64_t N,
                    int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int a_kmajor,
                    int b_kmajor, int epilogue_flags, const float* bias, const float* aux,
                    int64_t ldaux, void* workspace, size_t workspace_bytes,
                    molclr_stream_t stream);

/* molclr_gemm_f32 with the implementation chosen per call (tests and
 * benchmarks; molclr_gemm_f32 is impl = -1): -1 = automatic (split-bf16 "p6",
 * or "w6" for a long-K weight gradient), 0 = f32-input MFMA
 * (v_mfma_f32_32x32x2_f32), 64x64 tiles; 5 / 6 = split-bf16 "p6" (each fp32
 * operand split into 3 round-to-nearest bf16 parts, six bf16 MFMA products,
 * fp32 accumulation; fp32-GEMM accuracy), 64x64 / 128x64 tiles. */
int molclr_gemm_f32_impl(const float* A, const float* B, float* C, int64_t M, int64_t N,
                         int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int a_kmajor,
                         int b_kmajor, int epilogue_flags, const float* bias, const float* aux,
                         int64_t ldaux, void* workspace, size_t workspace_bytes,
                         molclr_stream_t stream, int impl);

/* Pre-split weight operand.  A Linear layer's weight is the B operand of the
 * forward (y = x W^T) and data-gradient (dx = dy W) GEMMs of every row tile;
 * splitting it once per optimizer step instead of once per row tile takes
 * half of the split work out of those GEMMs.
 *   molclr_bplanes_make: planes [3][Npad][Kp] bf16 (hi, mid, lo parts, the
 *     same split as the GEMM) of B(k, n) — stored like molclr_gemm_f32's B
 *     (b_kmajor: B[k*ldb + n], else B[n*ldb + k]) — zero-padded to
 *     Npad = N rounded up to 128, Kp = K rounded up to 32.
 *     molclr_bplanes_bytes(N, K) is their size.
 *   molclr_gemm_f32_bplanes: molclr_gemm_f32 with B given as such planes
 *     (same epilogues, split-K workspace from molclr_gemm_f32_workspace_bytes);
 *     a_kmajor needs M and lda multiples of 4, else K and lda. */
size_t molclr_bplanes_bytes(int64_t N, int64_t K);
int molclr_bplanes_make(const float* B, int64_t N, int64_t K, int64_t ldb, int b_kmajor,
                        uint16_t* planes, molclr_stream_t stream);
/* molclr_bplanes_make for `count` weights in one launch per 32 (host arrays of
 * per-weight arguments); the planes of a whole model after an optimizer step. */
int molclr_bplanes_make_batch(int count, const float* const* B, const int64_t* N,
                              const int64_t* K, const int64_t* ldb, const int* b_kmajor,
                              uint16_t* const* planes, molclr_stream_t stream);
int molclr_gemm_f32_bplanes(const float* A, const uint16_t* planes, float* C, int64_t M,
                            int64_t N, int64_t K, int64_t lda, int64_t ldc, int a_kmajor,
                            int epilogue_flags, const float* bias, const float* aux,
                            int64_t ldaux, void* workspace, size_t workspace_bytes,
                            molclr_stream_t stream);
/* molclr_gemm_f32_bplanes with the tile chosen per call (molclr_gemm_f32_bplanes
 * is tile = 0): 0 = automatic (9 for a row-major A whose 128-row tiles number
 * >= 128, else 64x128 for N >= 512, else 64x64), 5 = 64x64, 6 = 128x64,
 * 7 = 64x128, 8 = 128x128, 9 = "q6": 128 x 160 (or 128 / 64 wide) tiles with A
 * streamed through registers, one wave per 32 rows, for K <= 1024 (a K-major A
 * or a longer K falls back to 5 / 7). */
int molclr_gemm_f32_bplanes_tile(const float* A, const uint16_t* planes, float* C, int64_t M,
                                 int64_t N, int64_t K, int64_t lda, int64_t ldc, int a_kmajor,
                                 int epilogue_flags, const float* bias, const float* aux,
                                 int64_t ldaux, void* workspace, size_t workspace_bytes,
                                 molclr_stream_t stream, int tile);

/* Weight and bias gradients of y = x W^T + b (nn.Linear backward):
 *   dW[n_out][n_in] (+)= Σ_r dy[r][o] x[r][i],   db[n_out] (+)= Σ_r dy[r][o]
 * dy [rows, n_out] (row stride ld_dy), x [rows, n_in] (ld_x).  One split-bf16
 * GEMM that also takes the bias column sums from the dy tiles it stages (no
 * separate pass over dy).  db may be NULL; accumulate != 0 adds into dW / db.
 * db needs n_out and ld_dy multiples of 4.  Falls back to molclr_gemm_f32 +
 * molclr_colsum_f32 for shapes the fused kernel does not take. */
size_t molclr_linear_wgrad_workspace_bytes(int64_t rows, int64_t n_out, int64_t n_in);
int molclr_linear_wgrad(const float* dy, const float* x, float* dW, float* db, int64_t rows,
                        int64_t n_out, int64_t n_in, int64_t ld_dy, int64_t ld_x, int accumulate,
                        void* workspace, size_t workspace_bytes, molclr_stream_t stream);
/* molclr_linear_wgrad with the K groups per block of the long-K kernel chosen
 * per call (molclr_linear_wgrad is groups = 2): 2 = two 4-wave groups per block,
 * half as many split-K partial tiles; 1 = one group per block. */
int molclr_linear_wgrad_groups(const float* dy, const float* x, float* dW, float* db,
                               int64_t rows, int64_t n_out, int64_t n_in, int64_t ld_dy,
                               int64_t ld_x, int accumulate, void* workspace,
                               size_t workspace_bytes, molclr_stream_t stream, int groups);

/* "h3" fp32 GEMMs: three fp16 MFMA products per element pair instead of six
 * bf16 ones.  Each operand is scaled by a power of two chosen from its
 * tensor-wide max |x| (scaled max in [2^14, 2^15)) and split into two
 * round-to-nearest fp16 parts, x 2^s = hi + lo + t with |t| <= 2^-22 |x 2^s|;
 * hi_a hi_b + hi_a lo_b + lo_a hi_b accumulates in fp32 and is scaled back
 * exactly.  Same epilogues and shapes as the q6 / w6 kernels they replace
 * (models/ginet_molclr.py:19-23: the GIN MLP forward, data and weight
 * gradients).
 *   A max slot is 64 entries 128 bytes apart (2048 floats, 8 KB) whose max
 *     is the tensor's max |x| (producers spread their atomic maxima over the
 *     entries; atomics on one cache line serialise).
 *   molclr_absmax_f32: slot <- max |x| over a [rows][cols] (ld) matrix
 *     (accumulate != 0: folded into the current slot; else the slot is reset
 *     first).  The max is order-independent, so every producer of the same
 *     tensor gives the same slot value.
 *   molclr_hplanes_make_batch: weights as h3 B operands (molclr_bplanes_make_batch
 *     arguments): [2][Npad][Kp] fp16 planes, then the max |B| slot,
 *     molclr_hplanes_bytes(N, K) bytes each.
 *   molclr_absmax_rows_f32: rowmax[r] = max_c |x[r][c]| and the slot as
 *     molclr_absmax_f32.
 *   molclr_gemm_f32_h3: C = epilogue(A B) for a row-major A [M][K] (lda) and
 *     h3 planes of B; K <= 1024, K and lda multiples of 4.  a_row_parts == 0:
 *     `amax` is A's max slot (one scale for A); P > 0: `amax` holds A's row
 *     maxima as P partial arrays [P][M] (P < 0: as the per-wave pairs of
 *     molclr_rowmax_layout(K) = P) and every row is scaled by its own
 *     (a row of small values, e.g. a node with a small gradient, keeps full
 *     precision).  cmax / crow (each may be NULL): max |C| folded into the
 *     slot cmax (the caller zeroes it) / C's row maxima as
 *     molclr_gemm_row_parts(N) partial arrays (plain stores); amax_out (may
 *     be NULL, zeroed by the caller): max |A| folded in.  A RELU_MASK
 *     epilogue takes its mask from mask_bits (molclr_gemm_f32_bplanes_max's
 *     relu_bits of the same [M][N]) when given, else from aux.
 *   molclr_linear_wgrad_h3: molclr_linear_wgrad given the max slots of dy
 *     and x (n_out, n_in, ld_dy, ld_x multiples of 4; same workspace). */
int molclr_absmax_f32(const float* x, int64_t rows, int64_t cols, int64_t ld, float* slot,
                      int accumulate, molclr_stream_t stream);
size_t molclr_hplanes_bytes(int64_t N, int64_t K);
int molclr_hplanes_make_batch(int count, const float* const* B, const int64_t* N,
                              const int64_t* K, const int64_t* ldb, const int* b_kmajor,
                              uint16_t* const* planes, molclr_stream_t stream);
/* molclr_gemm_f32_bplanes (x6 planes, row-major A, K <= 1024; same kernel and
 * result as its automatic choice) that also folds max |A| of its A rows into
 * the slot amax_out and max |C| into the slot cmax (zeroed by the caller),
 * and writes C's row maxima as molclr_gemm_row_parts(N) partial arrays
 * crow[p][M] (plain stores; the row max is the max over p): the scales of
 * the h3 products that consume A or C, with no pass when the q6 kernel runs.
 * relu_bits: bit (n % 32) of word [n / 32][m] (ceil(N / 32) x M words) =
 * (C[m][n] > 0) -- the ReLU mask of a bias+ReLU product in 1/32 of the bytes.
 * Each output may be NULL. */
int64_t molclr_gemm_row_parts(int64_t N);
int molclr_gemm_f32_bplanes_max(const float* A, const uint16_t* planes, float* C, int64_t M,
                                int64_t N, int64_t K, int64_t lda, int64_t ldc,
                                int epilogue_flags, const float* bias, const float* aux,
                                int64_t ldaux, float* amax_out, float* cmax, float* crow,
                                uint32_t* relu_bits, void* workspace, size_t workspace_bytes,
                                molclr_stream_t stream);
int molclr_absmax_rows_f32(const float* x, int64_t rows, int64_t cols, int64_t ld,
                           float* rowmax, float* slot, int accumulate, molclr_stream_t stream);
int molclr_gemm_f32_h3(const float* A, const float* amax, int a_row_parts, const uint16_t* hplanes,
                       float* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldc,
                       int epilogue_flags, const float* bias, const float* aux, int64_t ldaux,
                       const uint32_t* mask_bits, float* cmax, float* crow, float* amax_out,
                       molclr_stream_t stream);
/* molclr_gemm_f32_h3_bits with the kernel chosen per call (tests): impl 0 =
 * automatic, 1 = k_gemm_pp / k_gemm_q6, 2 = k_gemm_bs, 3 = k_gemm_bs16 (both
 * bs: K in (288, 304], N > 320, C float4-aligned, ReLU mask as bits;
 * MOLCLR_ERR_UNSUPPORTED otherwise).  Kernels 1 and 2 give bit-identical C,
 * bits and maxima; 3 (16 x 16 x 32 MFMAs) sums each product's k in another
 * order, equal to fp32 rounding.  The row maxima (crow) are
 * molclr_gemm_row_parts(N) arrays whatever the kernel.  The bs kernels read
 * three wave words of per-wave-pair row maxima, so a product with
 * -a_row_parts > 129 (a row may span four waves, e.g. K = 600) is not theirs:
 * the automatic choice runs it on pp / q6, impl 2 / 3 answer UNSUPPORTED. */
int molclr_gemm_f32_h3_impl(const float* A, const float* amax, int a_row_parts,
                            const uint16_t* hplanes, float* C, int64_t M, int64_t N, int64_t K,
                            int64_t lda, int64_t ldc, int epilogue_flags, const float* bias,
                            const float* aux, int64_t ldaux, const uint32_t* mask_bits, float* cmax,
                            float* crow, float* amax_out, uint32_t* relu_bits,
                            molclr_stream_t stream, int impl);
/* molclr_gemm_f32_h3 whose BIAS_RELU product also writes C's ReLU mask as
 * bits (relu_bits: molclr_gemm_f32_bplanes_max's layout, may be NULL): the h3
 * forward's first GIN-MLP product, whose mask the dz1 product reads back. */
int molclr_gemm_f32_h3_bits(const float* A, const float* amax, int a_row_parts,
                            const uint16_t* hplanes, float* C, int64_t M, int64_t N, int64_t K,
                            int64_t lda, int64_t ldc, int epilogue_flags, const float* bias,
                            const float* aux, int64_t ldaux, const uint32_t* mask_bits,
                            float* cmax, float* crow, float* amax_out, uint32_t* relu_bits,
                            molclr_stream_t stream);
/* molclr_linear_wgrad_h3 with the K groups per block chosen per call (the plain
 * call is groups = 2), as molclr_linear_wgrad_groups. */
int molclr_linear_wgrad_h3_groups(const float* dy, const float* dymax, const float* x,
                                  const float* xmax, float* dW, float* db, int64_t rows,
                                  int64_t n_out, int64_t n_in, int64_t ld_dy, int64_t ld_x,
                                  int accumulate, void* workspace, size_t workspace_bytes,
                                  molclr_stream_t stream, int groups);
int molclr_linear_wgrad_h3(const float* dy, const float* dymax, const float* x,
                           const float* xmax, float* dW, float* db, int64_t rows, int64_t n_out,
                           int64_t n_in, int64_t ld_dy, int64_t ld_x, int accumulate,
                           void* workspace, size_t workspace_bytes, molclr_stream_t stream);
/* Two h3 weight gradients (a: dW_a = dy_a^T x_a, b likewise) over the same
 * row count, their ordered split-K reductions in ONE launch: the same results
 * as two molclr_linear_wgrad_h3 calls (rows >= 1024; sizes multiples of 4). */
size_t molclr_linear_wgrad_h3_pair_workspace_bytes(int64_t rows, int64_t n_out_a, int64_t n_in_a,
                                                   int64_t n_out_b, int64_t n_in_b);
int molclr_linear_wgrad_h3_pair(const float* dy_a, const float* dymax_a, const float* x_a,
                                const float* xmax_a, float* dW_a, float* db_a, int64_t n_out_a,
                                int64_t n_in_a, int64_t ld_dy_a, int64_t ld_x_a,
                                const float* dy_b, const float* dymax_b, const float* x_b,
                                const float* xmax_b, float* dW_b, float* db_b, int64_t n_out_b,
                                int64_t n_in_b, int64_t ld_dy_b, int64_t ld_x_b, int64_t rows,
                                int accumulate, void* workspace, size_t workspace_bytes,
                                molclr_stream_t stream);

/* out[n] = Σ_m X[m*ld + n]  (bias gradients), deterministic.
 * cols must be a multiple of 4 in [4, 4096] (one thread per float4 column, a
 * block of at most 1024 threads holds a whole row) and ld a multiple of 4:
 * any other width is MOLCLR_ERR_ARG, and its workspace query returns 0. */
size_t molclr_colsum_f32_workspace_bytes(int64_t rows, int64_t cols);
int molclr_colsum_f32(const float* X, float* out, int64_t rows, int64_t cols, int64_t ld,
                      int accumulate, void* workspace, size_t workspace_bytes,
                      molclr_stream_t stream);

/* ------------------------------------------------------------------------
 * BatchNorm1d over the rows of z [N,D] (+ ReLU), ginet_molclr.py:107-111.
 * training != 0: batch statistics (biased variance for normalising),
 *   running_mean/var updated in place with `momentum` and the unbiased
 *   variance, exactly as torch.nn.BatchNorm1d, and *num_batches_tracked
 *   (may be NULL) incremented; save_mean / save_invstd [D] receive the
 *   statistics for the backward.
 * training == 0: running statistics are used and nothing is updated.
 * relu != 0 applies max(y, 0) to the output.  y may be NULL: the statistics
 * (save_mean / save_invstd, running stats) are computed and the normalised
 * output is not written.
 * dim must be a multiple of 4 in [4, 4096] (the column-sum limit above), here
 * and in every molclr_batchnorm_seg_* call below: any other width is
 * MOLCLR_ERR_ARG, and its workspace query returns 0. */
size_t molclr_batchnorm_workspace_bytes(int64_t rows, int64_t dim);
int molclr_batchnorm_fwd(const float* z, const float* gamma, const float* beta,
                         float* running_mean, float* running_var,
                         int64_t* num_batches_tracked, float* y,
                         float* save_mean, float* save_invstd, int64_t rows, int64_t dim,
                         double momentum, double eps, int training, int relu,
                         void* workspace, size_t workspace_bytes, molclr_stream_t stream);
/* dy is the gradient w.r.t. the (ReLU'd) output; dz/dgamma/dbeta out. */
int molclr_batchnorm_bwd(const float* dy, const float* z, const float* gamma,
                         const float* beta, const float* save_mean,
                         const float* save_invstd, float* dz, float* dgamma, float* dbeta,
                         int64_t rows, int64_t dim, int relu, int accumulate, void* workspace,
                         size_t workspace_bytes, molclr_stream_t stream);

/* Segmented BatchNorm: the rows are `nseg` consecutive segments of
 * seg_rows[s] rows (host array), each normalised with its own batch statistics
 * -- the reference's two encoder calls per step (molclr.py:57,60) run as ONE
 * pass over both views -- and the running statistics updated once per
 * segment in segment order (num_batches_tracked += nseg).  Every segment's
 * outputs are bit-identical to a molclr_batchnorm_fwd / _bwd call over its
 * rows alone.  save_mean / save_invstd are [nseg, D].  dgamma / dbeta are the
 * sums over the segments (in segment order).  dtype: MOLCLR_DTYPE_F32 or
 * MOLCLR_DTYPE_BF16 storage of z / y / dy / dz (statistics always fp32). */
enum { MOLCLR_DTYPE_F32 = 0, MOLCLR_DTYPE_BF16 = 1 };
size_t molclr_batchnorm_seg_workspace_bytes(int nseg, const int64_t* seg_rows, int64_t dim);
int molclr_batchnorm_seg_fwd(const void* z, const float* gamma, const float* beta,
                             float* running_mean, float* running_var,
                             int64_t* num_batches_tracked, void* y, float* save_mean,
                             float* save_invstd, int nseg, const int64_t* seg_rows, int64_t dim,
                             int dtype, double momentum, double eps, int training, int relu,
                             void* workspace, size_t workspace_bytes, molclr_stream_t stream);
int molclr_batchnorm_seg_bwd(const void* dy, const void* z, const float* gamma,
                             const float* beta, const float* save_mean, const float* save_invstd,
                             void* dz, float* dgamma, float* dbeta, int nseg,
                             const int64_t* seg_rows, int64_t dim, int dtype, int relu,
                             int accumulate, void* workspace, size_t workspace_bytes,
                             molclr_stream_t stream);

/* molclr_batchnorm_seg_bwd (fp32; same dz) that also writes the row maxima of
 * dz as molclr_bn_row_parts(dim) partial arrays rowmax[p][rows] (plain
 * stores; max |dz[r]| = max over p) and folds max |dz| into the slot (may be
 * NULL; the caller zeroes it): the scales of the h3 products that consume dz
 * (molclr_gemm_f32_h3 row-wise, molclr_linear_wgrad_h3). */
int molclr_bn_row_parts(int64_t dim);
/* Device-sized segments (a captured step over padded buffers): the rows of
 * every segment are read from seg_rows_dev [nseg] on the device; z / y / dy /
 * dz hold rows_cap rows, and rows past the segments' sum are padding (y and dz
 * zero there, no statistics).  Same per-segment plan as the host-sized calls,
 * so the real rows' results are bit-identical to theirs.  The backward's
 * rowmax / slot (fp32 only, may be NULL) as molclr_batchnorm_seg_bwd_max. */
size_t molclr_batchnorm_seg_dev_workspace_bytes(int nseg, int64_t rows_cap, int64_t dim);
int molclr_batchnorm_seg_fwd_dev(const void* z, const float* gamma, const float* beta,
                                 float* running_mean, float* running_var,
                                 int64_t* num_batches_tracked, void* y, float* save_mean,
                                 float* save_invstd, int nseg, const int64_t* seg_rows_dev,
                                 int64_t rows_cap, int64_t dim, int dtype, double momentum,
                                 double eps, int training, int relu, void* workspace,
                                 size_t workspace_bytes, molclr_stream_t stream);
/* molclr_batchnorm_seg_fwd / _fwd_dev without the apply: the same partition
 * plan and kernels, the same save_mean / save_invstd, running statistics and
 * num_batches_tracked, and the apply coefficients left at coeffs (scale
 * [nseg,D], then shift [nseg,D]: y = fma(z, scale, shift)) for a consumer
 * that applies them itself (molclr_gine_aggregate_bn_fwd).  No y is written.
 * Workspace as the forward's. */
int molclr_batchnorm_seg_coeffs(const void* z, const float* gamma, const float* beta,
                                float* running_mean, float* running_var,
                                int64_t* num_batches_tracked, float* save_mean,
                                float* save_invstd, float* coeffs, int nseg,
                                const int64_t* seg_rows, int64_t dim, int dtype, double momentum,
                                double eps, int training, void* workspace, size_t workspace_bytes,
                                molclr_stream_t stream);
int molclr_batchnorm_seg_coeffs_dev(const void* z, const float* gamma, const float* beta,
                                    float* running_mean, float* running_var,
                                    int64_t* num_batches_tracked, float* save_mean,
                                    float* save_invstd, float* coeffs, int nseg,
                                    const int64_t* seg_rows_dev, int64_t rows_cap, int64_t dim,
                                    int dtype, double momentum, double eps, int training,
                                    void* workspace, size_t workspace_bytes,
                                    molclr_stream_t stream);
int molclr_batchnorm_seg_bwd_dev(const void* dy, const void* z, const float* gamma,
                                 const float* beta, const float* save_mean,
                                 const float* save_invstd, void* dz, float* dgamma, float* dbeta,
                                 int nseg, const int64_t* seg_rows_dev, int64_t rows_cap,
                                 int64_t dim, int dtype, int relu, int accumulate, float* rowmax,
                                 float* slot, void* workspace, size_t workspace_bytes,
                                 molclr_stream_t stream);
int molclr_batchnorm_seg_bwd_max(const float* dy, const float* z, const float* gamma,
                                 const float* beta, const float* save_mean,
                                 const float* save_invstd, float* dz, float* dgamma, float* dbeta,
                                 int nseg, const int64_t* seg_rows, int64_t dim, int relu,
                                 int accumulate, float* rowmax, float* slot, void* workspace,
                                 size_t workspace_bytes, molclr_stream_t stream);

/* The backward through frozen statistics: save_mean / save_invstd are the ones
 * an eval-mode forward (training = 0) saved, i.e. the running statistics.
 * dz = gamma * invstd * g does not depend on the column sums, so one pass over
 * dy and z stores dz and leaves the partial sums of dgamma / dbeta (same
 * partitions, same fixed order as the training-mode backward; no atomics).
 * Arguments, segment plans, rowmax / slot and workspace queries are those of
 * molclr_batchnorm_bwd / _seg_bwd / _seg_bwd_dev / _seg_bwd_max.  A segment
 * of one row is legal. */
int molclr_batchnorm_bwd_frozen(const float* dy, const float* z, const float* gamma,
                                const float* beta, const float* save_mean,
                                const float* save_invstd, float* dz, float* dgamma,
                                float* dbeta, int64_t rows, int64_t dim, int relu,
                                int accumulate, void* workspace, size_t workspace_bytes,
                                molclr_stream_t stream);
int molclr_batchnorm_seg_bwd_frozen(const void* dy, const void* z, const float* gamma,
                                    const float* beta, const float* save_mean,
                                    const float* save_invstd, void* dz, float* dgamma,
                                    float* dbeta, int nseg, const int64_t* seg_rows, int64_t dim,
                                    int dtype, int relu, int accumulate, void* workspace,
                                    size_t workspace_bytes, molclr_stream_t stream);
int molclr_batchnorm_seg_bwd_frozen_dev(const void* dy, const void* z, const float* gamma,
                                        const float* beta, const float* save_mean,
                                        const float* save_invstd, void* dz, float* dgamma,
                                        float* dbeta, int nseg, const int64_t* seg_rows_dev,
                                        int64_t rows_cap, int64_t dim, int dtype, int relu,
                                        int accumulate, float* rowmax, float* slot,
                                        void* workspace, size_t workspace_bytes,
                                        molclr_stream_t stream);
int molclr_batchnorm_seg_bwd_frozen_max(const float* dy, const float* z, const float* gamma,
                                        const float* beta, const float* save_mean,
                                        const float* save_invstd, float* dz, float* dgamma,
                                        float* dbeta, int nseg, const int64_t* seg_rows,
                                        int64_t dim, int relu, int accumulate, float* rowmax,
                                        float* slot, void* workspace, size_t workspace_bytes,
                                        molclr_stream_t stream);

/* Segment pooling over graph_ptr (PyG global_mean_pool / global_add_pool):
 * mode 0 = mean (sum / max(count,1)), 1 = add. */
int molclr_segment_pool_fwd(const float* h, const int32_t* graph_ptr, float* out,
                            int64_t num_graphs, int64_t dim, int mode,
                            molclr_stream_t stream);
int molclr_segment_pool_bwd(const float* dout, const int32_t* graph_ptr, float* dh,
                            int64_t num_nodes, int64_t num_graphs, int64_t dim, int mode,
                            molclr_stream_t stream);
/* global_max_pool (models/ginet_molclr.py:85-86, gcn_molclr.py:125-126: PyG
 * 1.6.3 -> torch_scatter 2.0.6 scatter_max).  out[g][d] = max over the nodes
 * of graph g, argmax[g][d] = that node (the first in node order among equal
 * values; -1 and out = 0 for a graph without nodes).  h is fp32 or bf16
 * (dtype MOLCLR_DTYPE_*), out / dout fp32; the backward writes dout[g][d] to
 * dh[argmax[g][d]][d] and zero elsewhere (dh in h's dtype).  D % 4 == 0. */
int molclr_segment_max_fwd(const void* h, const int32_t* graph_ptr, float* out, int32_t* argmax,
                           int64_t num_graphs, int64_t dim, int dtype, molclr_stream_t stream);
int molclr_segment_max_bwd(const float* dout, const int32_t* argmax, void* dh, int64_t num_nodes,
                           int64_t num_graphs, int64_t dim, int dtype, molclr_stream_t stream);

/* F.normalize(z, dim=1, eps): y = z / max(||z||, eps); norm [rows] saved. */
int molclr_l2norm_fwd(const float* z, float* y, float* norm, int64_t rows, int64_t dim,
                      double eps, molclr_stream_t stream);
int molclr_l2norm_bwd(const float* dy, const float* y, const float* norm, float* dz,
                      int64_t rows, int64_t dim, double eps, molclr_stream_t stream);

/* ------------------------------------------------------------------------
 * NT-Xent (utils/nt_xent.py:47-65), row-sharded so it also serves the
 * data-parallel global batch.
 *   R = [zj ; zi] in the global order (nt_xent.py:48), 2B rows of width C.
 *   cosine != 0: rows are first scaled by 1/max(||r||, 1e-8)
 *       (torch CosineSimilarity, nt_xent.py:40-45); cosine == 0: dot.
 *   loss = (1/2B) Σ_r [ log Σ_{c≠r} exp(S_rc/T) − S_{r,(r+B) mod 2B}/T ].
 * This process owns `nrows` rows of R: `rows` [nrows,C] with global indices
 * row_gidx [nrows]; `cols` [2B,C] is the full (gathered) R.
 * ntxent_prep: rhat = scaled rows of a [n,C] matrix, norm [n] (clamped denominators).
 * ntxent_fwd:  lse_rows [nrows] (needed by every rank's backward) and
 *              loss_rows [nrows] = per-row loss / 2B.
 * ntxent_bwd:  drhat_rows [nrows,C] = dL/d(rhat rows) given the full
 *              lse_cols [2B] and the upstream scalar gradient *grad_loss.
 * ntxent_prep_bwd: chain rule through the row scaling. */
int molclr_ntxent_prep(const float* r, float* rhat, float* norm, int64_t n, int64_t C,
                       int cosine, molclr_stream_t stream);
int molclr_ntxent_prep_bwd(const float* drhat, const float* rhat, const float* norm,
                           float* dr, int64_t n, int64_t C, int cosine,
                           molclr_stream_t stream);
/* The paired step's F.normalize (molclr.py:63-64, eps) and ntxent_prep in one
 * launch, replacing l2norm_fwd + torch.cat([zjs, zis]) + ntxent_prep
 * (GINet.forward_pair's z = [zis; zjs], 2 * batch_local rows):
 *   rhat [2Bl,C] = scaled rows of R = [zjs; zis], y [2Bl,C] the normalised R,
 *   n1 [2Bl] = |R row| (unclamped, as l2norm_fwd's norm), n2 [2Bl] the clamped
 *   cosine denominator (1 for dot similarity).  Bit-identical to the three ops.
 * ntxent_prep_pair_bwd: dz [2Bl,C] in z's row order from drhat. */
int molclr_ntxent_prep_pair(const float* z, float* y, float* rhat, float* n1, float* n2,
                            int64_t batch_local, int64_t C, double eps, int cosine,
                            molclr_stream_t stream);
int molclr_ntxent_prep_pair_bwd(const float* drhat, const float* rhat, const float* n2,
                                const float* y, const float* n1, float* dz, int64_t batch_local,
                                int64_t C, double eps, int cosine, molclr_stream_t stream);
size_t molclr_ntxent_workspace_bytes(int64_t nrows, int64_t ncols, int64_t C);
int molclr_ntxent_fwd(const float* rhat_rows, const int32_t* row_gidx, const float* rhat_cols,
                      int64_t nrows, int64_t ncols, int64_t C, int64_t batch_size,
                      double temperature, float* lse_rows, float* loss_rows,
                      void* workspace, size_t workspace_bytes, molclr_stream_t stream);
int molclr_ntxent_bwd(const float* rhat_rows, const int32_t* row_gidx, const float* rhat_cols,
                      const float* lse_cols, const float* grad_loss, int64_t nrows,
                      int64_t ncols, int64_t C, int64_t batch_size, double temperature,
                      float* drhat_rows, void* workspace, size_t workspace_bytes,
                      molclr_stream_t stream);
/* molclr_ntxent_fwd / _bwd with the formulation chosen per call (tests and
 * benchmarks; -1 = automatic, as the calls above): 0 = fused f32-MFMA kernels
 * (similarity tiles recomputed in registers, online logsumexp, no S buffer);
 * 1 = S = rows cols^T as one split-bf16 GEMM (fp32 accuracy), then the row
 * logsumexp / the symmetric weights W as elementwise passes and dR = W cols as
 * a second GEMM (ncols % 4 == 0); 2 = the h3 form of 1 (S by three fp16
 * MFMAs per product, W^T through an LDS transpose, dR as an h3 weight-gradient
 * product; nrows, ncols, C % 4 == 0, C <= 1024, ncols >= 1024); 3 = the
 * transposed form of 2 (S^T = cols rows^T kept [ncols][nrows], the row
 * logsumexp down its columns, W^T elementwise in S^T's layout: no transpose
 * pass; same shapes as 2).  Automatic: 0
 * below 2^20 elements of S, 1 up to 2^22, 2 from there where its shapes allow.
 * sim (formulations 1, 2, 3; may be NULL): the forward writes row-major S
 * [nrows][ncols] there (1 and 2) or S^T [ncols][nrows] (3), and a backward given the same
 * buffer uses it instead of recomputing S.  molclr_ntxent_sim_bytes: its
 * size, 0 when the formulation chosen for (nrows, ncols, C, impl) keeps no S. */
size_t molclr_ntxent_sim_bytes(int64_t nrows, int64_t ncols, int64_t C, int impl);
int molclr_ntxent_fwd_impl(const float* rhat_rows, const int32_t* row_gidx,
                           const float* rhat_cols, int64_t nrows, int64_t ncols, int64_t C,
                           int64_t batch_size, double temperature, float* lse_rows,
                           float* loss_rows, float* sim, void* workspace, size_t workspace_bytes,
                           molclr_stream_t stream, int impl);
int molclr_ntxent_bwd_impl(const float* rhat_rows, const int32_t* row_gidx,
                           const float* rhat_cols, const float* lse_cols, const float* grad_loss,
                           int64_t nrows, int64_t ncols, int64_t C, int64_t batch_size,
                           double temperature, const float* sim, float* drhat_rows,
                           void* workspace, size_t workspace_bytes, molclr_stream_t stream,
                           int impl);
/* loss = Σ loss_rows (deterministic single-block sum). */
int molclr_sum_f32(const float* x, float* out, int64_t n, molclr_stream_t stream);

/* ------------------------------------------------------------------------
 * Adam with coupled L2 weight decay over one flat fp32 parameter buffer
 * (torch.optim.Adam semantics, molclr.py:84-87,127):
 *   g += wd·p; m = b1·m + (1−b1)·g; v = b2·v + (1−b2)·g²;
 *   p −= lr/(1−b1^t) · m / (sqrt(v)/sqrt(1−b2^t) + eps)
 * lr and step live in device memory so a captured step replays with the
 * current learning rate; *step is incremented by the kernel. */
int molclr_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                     int64_t n, const float* lr, int32_t* step, double beta1, double beta2,
                     double eps, double weight_decay, molclr_stream_t stream);
/* molclr_adam_step with tick = 0 leaves the step counter alone (the update
 * uses *step + 1 as always): molclr_step_tail then advances it, and also
 * copies the loss scalar and ORs the batch's status word into a sticky word
 * (either may be NULL) -- the HIP-graph step's single closing launch. */
int molclr_adam_step_ex(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                        int64_t n, const float* lr, int32_t* step, double beta1, double beta2,
                        double eps, double weight_decay, int tick, molclr_stream_t stream);
int molclr_step_tail(int32_t* step, const float* loss_src, float* loss_dst,
                     const int32_t* status_src, int32_t* status_acc, molclr_stream_t stream);

/* ------------------------------------------------------------------------
 * GIN encoder executor (models/ginet_molclr.py:98-111 as ONE call).
 * Runs the whole node-embedding stack of GINet on the stream — atom
 * embedding, then per layer GINE aggregation -> Linear(D,2D)+ReLU ->
 * Linear(2D,D) -> BatchNorm1d (+ReLU, not on the last layer) — by calling
 * the entry points above in the order molclr_amd's per-op autograd path
 * calls them (identical kernels, identical results), without a host round
 * trip per operation.  The backward call replays the layers in reverse and
 * ADDS every parameter gradient into the given buffers.
 * Parameters are the reference's (state_dict names in the fields); the four
 * *_planes are molclr_bplanes_make images of the MLP weights as GEMM B
 * operands:
 *   mlp0_planes   : B(k,n) = W0[n][k], N = 2D, K = D   (ldb = D,  b_kmajor 0)
 *   mlp0_planes_t : B(k,n) = W0[k][n], N = D,  K = 2D  (ldb = D,  b_kmajor 1)
 *   mlp2_planes   : B(k,n) = W2[n][k], N = D,  K = 2D  (ldb = 2D, b_kmajor 0)
 *   mlp2_planes_t : B(k,n) = W2[k][n], N = 2D, K = D   (ldb = 2D, b_kmajor 1)
 * BatchNorm: training = batch statistics + running-stat update (momentum,
 * num_batches_tracked may be NULL); eval = running statistics (no backward).
 * Dropout (training and drop_ratio > 0; the reference's F.dropout after every
 * BatchNorm, after the ReLU where there is one): a counter-based mask (see
 * molclr_dropout_mask) recomputed wherever a layer's output is used -- the
 * apply that stores it, the next layer's gather, the BatchNorm backward -- so
 * it costs no buffer and one extra launch per forward: the forward's first
 * launch is molclr_dropout_next_key(drop_state, <the arena's key slot>), and
 * every kernel of that forward and of its backward reads the key from the
 * arena.  A backward therefore sees its own forward's masks however many
 * forwards ran in between, and a replayed HIP graph draws fresh masks.
 * ------------------------------------------------------------------------ */
/* The `training` field of both encoder structs. */
enum {
  MOLCLR_MODE_EVAL = 0,      /* running statistics, no dropout */
  MOLCLR_MODE_TRAIN = 1,     /* batch statistics, running statistics updated, dropout */
  MOLCLR_MODE_FROZEN_BN = 2  /* running statistics, nothing updated
                              * (num_batches_tracked included), dropout as in training */
};
typedef struct molclr_gin_encoder {
  int32_t num_layer;  /* 1 .. MOLCLR_MAX_LAYERS */
  int32_t training;   /* MOLCLR_MODE_*; the backward runs in every mode */
  int64_t dim;        /* emb_dim, multiple of 4 */
  int64_t n_atom;     /* x_embedding1 rows (119) */
  int64_t n_chiral;   /* x_embedding2 rows (3) */
  double momentum, eps;
  const float* x_embedding1;
  const float* x_embedding2;
  const float* mlp0_weight[MOLCLR_MAX_LAYERS];
  const float* mlp0_bias[MOLCLR_MAX_LAYERS];
  const float* mlp2_weight[MOLCLR_MAX_LAYERS];
  const float* mlp2_bias[MOLCLR_MAX_LAYERS];
  const float* edge_embedding1[MOLCLR_MAX_LAYERS];
  const float* edge_embedding2[MOLCLR_MAX_LAYERS];
  const float* bn_weight[MOLCLR_MAX_LAYERS];
  const float* bn_bias[MOLCLR_MAX_LAYERS];
  float* bn_running_mean[MOLCLR_MAX_LAYERS];
  float* bn_running_var[MOLCLR_MAX_LAYERS];
  int64_t* bn_num_batches_tracked[MOLCLR_MAX_LAYERS];
  const uint16_t* mlp0_planes[MOLCLR_MAX_LAYERS];
  const uint16_t* mlp0_planes_t[MOLCLR_MAX_LAYERS];
  const uint16_t* mlp2_planes[MOLCLR_MAX_LAYERS];
  const uint16_t* mlp2_planes_t[MOLCLR_MAX_LAYERS];
  /* MOLCLR_DTYPE_F32: fp32 node features, split-bf16 GEMMs (fp32 accuracy).
   * MOLCLR_DTYPE_BF16 (dim % 8 == 0): bf16 node features and activation
   * gradients, one bf16 MFMA per product with fp32 accumulation (plane 0 of
   * the *_planes images is the bf16 weight), fp32 statistics, tables, and
   * parameter gradients: the c5 configuration / the reference's
   * mixed-precision switch (molclr.py:16-24,93-96,121-123).  h_out / dh_out
   * are then bf16. */
  int32_t dtype;
  /* fp32 storage only, which products run in "h3" (molclr_gemm_f32_h3 /
   * molclr_linear_wgrad_h3, 2 dim <= 1024) instead of split-bf16 "x6":
   * 0 = none; bit 0 = the backward (weight gradients with per-tensor scales,
   * data gradients with row-wise scales; mlp*_planes_t are then
   * molclr_hplanes_make_batch images); bit 1 = the forward products too
   * (mlp0/2_planes h3 images, A scaled row by row; the Python side's default,
   * 3 = both).  The max slots of agg / a1 live in the arena, those of dz /
   * dz1 and all row maxima in the workspace. */
  int32_t fp32_gemm;
  /* nullable: receives MOLCLR_STATUS_ATOM_RANGE (molclr_atom_embed_fwd) */
  int32_t* status;
  /* dropout after every BatchNorm: 0 <= drop_ratio < 1; drop_state: device
   * [seed, call counter] (NULL allowed unless training with drop_ratio > 0).
   * Both are ignored in eval mode. */
  double drop_ratio;
  int64_t* drop_state;
} molclr_gin_encoder;

/* Gradient buffers, same shapes as the parameters; NULL = not needed. */
typedef struct molclr_gin_encoder_grads {
  float* x_embedding1;
  float* x_embedding2;
  float* mlp0_weight[MOLCLR_MAX_LAYERS];
  float* mlp0_bias[MOLCLR_MAX_LAYERS];
  float* mlp2_weight[MOLCLR_MAX_LAYERS];
  float* mlp2_bias[MOLCLR_MAX_LAYERS];
  float* edge_embedding1[MOLCLR_MAX_LAYERS];
  float* edge_embedding2[MOLCLR_MAX_LAYERS];
  float* bn_weight[MOLCLR_MAX_LAYERS];
  float* bn_bias[MOLCLR_MAX_LAYERS];
  /* Optional (NULL = none): hipEvent_t handles the backward records on its
   * stream once layer l's parameter gradients (its Linear / GCN weights,
   * edge tables and BatchNorm affine) are final, and once the atom-embedding
   * gradients are: a data-parallel caller starts each layer's gradient
   * all-reduce behind its event while the lower layers' backward runs. */
  void* layer_done[MOLCLR_MAX_LAYERS];
  void* embed_done;
} molclr_gin_encoder_grads;

/* The graph of one batch as molclr_graph_build produced it. */
/* num_segments > 1: the graph is molclr_graph_build_multi's union of that many
 * batches with segment_nodes[s] nodes each; the executors keep the
 * BatchNorm statistics of every segment apart (molclr_batchnorm_seg_fwd).
 * num_segments 0 or 1: one batch. */
typedef struct molclr_device_graph {
  int64_t num_nodes, num_edges, num_graphs;
  const int32_t *rowptr, *col, *rowptr_t, *col_t, *ecount, *graph_ptr;
  const uint8_t* ecode;
  const uint32_t *nbr, *nbr_t;
  int32_t num_segments;
  int64_t segment_nodes[MOLCLR_MAX_SEGMENTS];
  /* NULL, or (molclr_graph_build_dev) the segments' node counts on the device:
   * num_nodes is then the capacity, segment_nodes is unused and the rows past
   * the counts' sum are padding */
  const int64_t* segment_nodes_dev;
} molclr_device_graph;

/* Saved activations of one forward (kept for the backward): arena of
 * molclr_gin_encoder_arena_bytes; scratch: molclr_gin_encoder_workspace_bytes. */
size_t molclr_gin_encoder_arena_bytes(int num_layer, int64_t num_nodes, int64_t dim, int dtype);
size_t molclr_gin_encoder_workspace_bytes(int num_layer, int64_t num_nodes, int64_t dim,
                                          int dtype);
/* x int64 [N,2] (atom type, chirality); h_out [N,D] (enc->dtype): the last
 * BatchNorm's output. */
int molclr_gin_encoder_fwd(const molclr_gin_encoder* enc, const int64_t* x,
                           const molclr_device_graph* graph, void* h_out, void* arena,
                           size_t arena_bytes, void* workspace, size_t workspace_bytes,
                           molclr_stream_t stream);
/* dh_out [N,D] (enc->dtype): gradient w.r.t. h_out; grads are accumulated (+=). */
int molclr_gin_encoder_bwd(const molclr_gin_encoder* enc, const molclr_gin_encoder_grads* grads,
                           const int64_t* x, const molclr_device_graph* graph,
                           const void* dh_out, const void* arena, size_t arena_bytes,
                           void* workspace, size_t workspace_bytes, molclr_stream_t stream);

/* GCN encoder executor: GCN's node-embedding stack (models/gcn_molclr.py:140-151:
 * atom embedding, per layer GCNConv -> BatchNorm1d (+ReLU but the last)) in one
 * host call per direction, issuing the same entry points as the per-op path
 * (molclr_amd.ops: gemm_w, molclr_gcn_aggregate_fwd/_bwd, batchnorm, gemm) in
 * its order, so the results are identical.  weight[l] is GCNConv.weight
 * [D_in, D_out] (not transposed, gcn_molclr.py:45); weight_planes[l] its planes
 * as the B operand of x W (molclr_bplanes_make(W, D, D, D, b_kmajor=1)),
 * weight_planes_t[l] as the B operand of dxw W^T (b_kmajor=0). */
typedef struct molclr_gcn_encoder {
  int32_t num_layer;
  int32_t training; /* MOLCLR_MODE_* */
  int64_t dim;
  int64_t n_atom;
  int64_t n_chiral;
  double momentum, eps;
  const float* x_embedding1;
  const float* x_embedding2;
  const float* weight[MOLCLR_MAX_LAYERS];
  const float* bias[MOLCLR_MAX_LAYERS];
  const float* edge_embedding1[MOLCLR_MAX_LAYERS]; /* [5,1] */
  const float* edge_embedding2[MOLCLR_MAX_LAYERS]; /* [3,1] */
  const float* bn_weight[MOLCLR_MAX_LAYERS];
  const float* bn_bias[MOLCLR_MAX_LAYERS];
  float* bn_running_mean[MOLCLR_MAX_LAYERS];
  float* bn_running_var[MOLCLR_MAX_LAYERS];
  int64_t* bn_num_batches_tracked[MOLCLR_MAX_LAYERS];
  const uint16_t* weight_planes[MOLCLR_MAX_LAYERS];
  const uint16_t* weight_planes_t[MOLCLR_MAX_LAYERS];
  /* 0 = split-bf16 x6 products; 1 = the backward in h3 (as molclr_gin_encoder's
   * bit 0: the weight gradient with per-tensor scales, dx = dxw W^T with
   * row-wise scales; weight_planes_t are then molclr_hplanes_make_batch
   * images, dim <= 1024).  fp32 storage only. */
  int32_t fp32_gemm;
  /* MOLCLR_DTYPE_F32 (0, so a zero-initialised struct): fp32 node features.
   * MOLCLR_DTYPE_BF16 (dim % 8 == 0, fp32_gemm 0): bf16 node features and
   * activation gradients -- x W and dxw W^T as one bf16 MFMA per product on
   * plane 0 of weight_planes / weight_planes_t (molclr_gemm_bf16), the bf16
   * aggregation and BatchNorm, dW through molclr_linear_wgrad_bf16; fp32
   * statistics, tables, bias and parameter gradients: the reference's
   * mixed-precision switch for the GCN (molclr.py:16-24,93-96,
   * finetune.py:180-183).  h_out / dh_out are then bf16.  The field lies in
   * what was the padding between fp32_gemm and status: the size of the struct
   * and the offset of every other field are unchanged. */
  int32_t dtype;
  int32_t* status; /* nullable: MOLCLR_STATUS_ATOM_RANGE, as molclr_gin_encoder */
  double drop_ratio;   /* as molclr_gin_encoder */
  int64_t* drop_state; /* as molclr_gin_encoder */
} molclr_gcn_encoder;

typedef struct molclr_gcn_encoder_grads {
  float* x_embedding1;
  float* x_embedding2;
  float* weight[MOLCLR_MAX_LAYERS];
  float* bias[MOLCLR_MAX_LAYERS];
  float* edge_embedding1[MOLCLR_MAX_LAYERS];
  float* edge_embedding2[MOLCLR_MAX_LAYERS];
  float* bn_weight[MOLCLR_MAX_LAYERS];
  float* bn_bias[MOLCLR_MAX_LAYERS];
  void* layer_done[MOLCLR_MAX_LAYERS]; /* as in molclr_gin_encoder_grads */
  void* embed_done;
} molclr_gcn_encoder_grads;

/* Arena (the activations one forward saves for its backward) and workspace
 * (scratch) of an fp32 encoder (dtype MOLCLR_DTYPE_F32) ... */
size_t molclr_gcn_encoder_arena_bytes(int num_layer, int64_t num_nodes, int64_t dim);
size_t molclr_gcn_encoder_workspace_bytes(int num_layer, int64_t num_nodes, int64_t dim);
/* ... and of an encoder of either storage type (0 for an unknown dtype). */
size_t molclr_gcn_encoder_arena_bytes_dtype(int num_layer, int64_t num_nodes, int64_t dim,
                                            int dtype);
size_t molclr_gcn_encoder_workspace_bytes_dtype(int num_layer, int64_t num_nodes, int64_t dim,
                                                int dtype);
/* h_out / dh_out [N,D] in enc->dtype storage, as molclr_gin_encoder_fwd / _bwd. */
int molclr_gcn_encoder_fwd(const molclr_gcn_encoder* enc, const int64_t* x,
                           const molclr_device_graph* graph, void* h_out, void* arena,
                           size_t arena_bytes, void* workspace, size_t workspace_bytes,
                           molclr_stream_t stream);
int molclr_gcn_encoder_bwd(const molclr_gcn_encoder* enc, const molclr_gcn_encoder_grads* grads,
                           const int64_t* x, const molclr_device_graph* graph,
                           const void* dh_out, const void* arena, size_t arena_bytes,
                           void* workspace, size_t workspace_bytes, molclr_stream_t stream);

/* ------------------------------------------------------------------------
 * The executors' dropout stream.  Philox4x32-10 (multipliers 0xD2511F53 /
 * 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85), one call per float4
 * column unit: counter (row, column / 4, layer, call_lo), key (seed_lo,
 * seed_hi ^ call_hi); output word j decides column 4 (column / 4) + j.  An
 * element is kept iff word >= (uint32_t)(p * 2^32); kept elements are
 * multiplied by 1 / (1 - p), dropped ones are exactly 0.  `row` is the row of
 * the graph the executor sees (both views' rows in a paired pass).
 * ------------------------------------------------------------------------ */
/* key_out[0..1] = state[0..1] = (seed, call counter), then counter += 1; one
 * one-thread launch, all on the device. */
int molclr_dropout_next_key(int64_t* state, int64_t* key_out, molclr_stream_t stream);
/* keep [N, D] (D a multiple of 4): 1 where layer `layer`'s dropout with
 * probability p keeps the element under `key` (device [seed, call]), else 0;
 * computed by the device function the executors' kernels use. */
int molclr_dropout_mask(const int64_t* key, int layer, double p, uint8_t* keep, int64_t N,
                        int64_t D, molclr_stream_t stream);

/* ------------------------------------------------------------------------
 * bf16 storage (BASELINE config c5: GIN 5 x 512, bf16, batch 1024 / GPU).
 * Node features and activation gradients are bf16 ([N,D] of uint16 bit
 * patterns, round-to-nearest-even); all arithmetic, tables, statistics and
 * parameter gradients are fp32.  Same semantics as the fp32 entry points.
 * The GCN's bf16 entry points (molclr_gcn_aggregate_fwd_bf16 / _bwd_bf16) are
 * declared next to their fp32 forms; molclr_gcn_encoder.dtype selects the
 * storage of its executor.
 * ------------------------------------------------------------------------ */
int molclr_atom_embed_fwd_bf16(const int64_t* x, const float* X1, const float* X2, uint16_t* h,
                               int64_t num_nodes, int64_t dim, int64_t n1, int64_t n2,
                               int32_t* status, molclr_stream_t stream);
/* workspace: molclr_atom_embed_bwd_workspace_bytes */
int molclr_atom_embed_bwd_bf16(const int64_t* x, const uint16_t* dh, float* dX1, float* dX2,
                               int64_t num_nodes, int64_t dim, int64_t n1, int64_t n2,
                               int accumulate, void* workspace, size_t workspace_bytes,
                               molclr_stream_t stream);
int molclr_gine_aggregate_fwd_bf16(const uint16_t* x, const int32_t* rowptr, const int32_t* col,
                                   const uint8_t* ecode, const uint32_t* nbr, const float* Ec,
                                   uint16_t* out, int64_t num_nodes, int64_t dim,
                                   molclr_stream_t stream);
/* molclr_gine_aggregate_bn_fwd over bf16 storage: z, out bf16; every source
 * element is the apply's y rounded to bf16 (as stored) and widened again. */
int molclr_gine_aggregate_bn_fwd_bf16(const uint16_t* z, const float* coeffs, int relu, int nseg,
                                      const int64_t* seg_rows, const int64_t* seg_rows_dev,
                                      const int32_t* rowptr, const int32_t* col,
                                      const uint8_t* ecode, const uint32_t* nbr, const float* Ec,
                                      uint16_t* out, int64_t N, int64_t D,
                                      molclr_stream_t stream);
/* workspace: molclr_gine_aggregate_bwd_workspace_bytes */
int molclr_gine_aggregate_bwd_bf16(const uint16_t* g, const int32_t* rowptr_t,
                                   const int32_t* col_t, const uint32_t* nbr_t,
                                   const int32_t* ecount, uint16_t* dx, float* dE1, float* dE2,
                                   int64_t num_nodes, int64_t dim, int accumulate, void* workspace,
                                   size_t workspace_bytes, molclr_stream_t stream);
/* h bf16 -> out fp32 [G,D]; dout fp32 -> dh bf16 */
int molclr_segment_pool_fwd_bf16(const uint16_t* h, const int32_t* graph_ptr, float* out,
                                 int64_t num_graphs, int64_t dim, int mode,
                                 molclr_stream_t stream);
int molclr_segment_pool_bwd_bf16(const float* dout, const int32_t* graph_ptr, uint16_t* dh,
                                 int64_t num_nodes, int64_t num_graphs, int64_t dim, int mode,
                                 molclr_stream_t stream);
/* C[M,N] (bf16) = epilogue(Σ_k A[m][k] B(k,n)), A bf16 row-major (lda), B the
 * weight operand as molclr_bplanes_make planes (plane 0 = bf16(B) is read),
 * one v_mfma_f32_32x32x16_bf16 per product, fp32 accumulation.  Epilogues:
 * NONE / BIAS / BIAS_RELU (bias fp32) / RELU_MASK (aux bf16, ldaux % 4 == 0);
 * no accumulate.  K and lda multiples of 8, ldc a multiple of 4. */
int molclr_gemm_bf16(const uint16_t* A, const uint16_t* planes, uint16_t* C, int64_t M, int64_t N,
                     int64_t K, int64_t lda, int64_t ldc, int epilogue, const float* bias,
                     const uint16_t* aux, int64_t ldaux, molclr_stream_t stream);
/* The same with the tile shape chosen per call (tests and benchmarks; -1 =
 * automatic, as molclr_gemm_bf16): output tiles 0 = 128 x 128, 1 = 128 x 256,
 * 2 = 128 x 512, 3 = 64 x 512, 4 = 128 x 256 (8 waves), 5 = 128 x 128 (shallow
 * A prefetch), 6 = 256 x 256 with LDS-DMA staging (K % 64 == 0), 7 = 256 x 256
 * with a four-stage LDS-DMA ring (K % 32 == 0), 8 = 6 as a persistent kernel
 * (one block per CU, epilogue overlapped with the next tile's staging; K % 64
 * == 0); 6, 7 and 8 fall back to 2 for other K.  Every shape gives the same
 * result bits (those of hipBLASLt's bf16
 * GEMM on the epilogue-free products). */
int molclr_gemm_bf16_impl(const uint16_t* A, const uint16_t* planes, uint16_t* C, int64_t M,
                          int64_t N, int64_t K, int64_t lda, int64_t ldc, int epilogue,
                          const float* bias, const uint16_t* aux, int64_t ldaux,
                          molclr_stream_t stream, int impl);
/* molclr_gemm_bf16 (the persistent 256 x 256 kernel; K % 64 == 0) with the
 * ReLU mask as bits -- column-block-major words bits[n / 32][m], bit n % 32 =
 * (C[m][n] > 0), ceil(N / 32) x M words (molclr_gemm_f32_bplanes_max's
 * layout): epilogue MOLCLR_EPI_BIAS_RELU writes them to bits_out (the GIN
 * MLP's first Linear, ginet_molclr.py:19-23), MOLCLR_EPI_RELU_MASK takes its
 * mask from bits_in instead of a bf16 aux matrix (the ReLU backward): 1/16 of
 * the mask bytes.  Results equal the aux form's bit for bit. */
int molclr_gemm_bf16_bits(const uint16_t* A, const uint16_t* planes, uint16_t* C, int64_t M,
                          int64_t N, int64_t K, int64_t lda, int64_t ldc, int epilogue,
                          const float* bias, uint32_t* bits_out, const uint32_t* bits_in,
                          molclr_stream_t stream);
/* Linear weight / bias gradients from bf16 operands into fp32:
 * dW[n_out][n_in] (+)= Σ_r dy[r][o] x[r][i], db (+)= Σ_r dy[r][o] (db may be
 * NULL); n_out, n_in, ld_dy, ld_x multiples of 8.  Split-K partials summed in
 * a fixed order (deterministic). */
size_t molclr_linear_wgrad_bf16_workspace_bytes(int64_t rows, int64_t n_out, int64_t n_in);
int molclr_linear_wgrad_bf16(const uint16_t* dy, const uint16_t* x, float* dW, float* db,
                             int64_t rows, int64_t n_out, int64_t n_in, int64_t ld_dy,
                             int64_t ld_x, int accumulate, void* workspace,
                             size_t workspace_bytes, molclr_stream_t stream);
/* The same with the kernel chosen per call (-1 = automatic): 0 = 128 x 128,
 * 1 = 256 x 256, 2 = 128 x 256 output tiles with register staging, 3 = 256 x
 * 256 with both operands LDS-DMA staged (64-row K steps); each has its own
 * split-K plan (the workspace query covers all). */
int molclr_linear_wgrad_bf16_impl(const uint16_t* dy, const uint16_t* x, float* dW, float* db,
                                  int64_t rows, int64_t n_out, int64_t n_in, int64_t ld_dy,
                                  int64_t ld_x, int accumulate, void* workspace,
                                  size_t workspace_bytes, molclr_stream_t stream, int impl);

/* ---- Supervised task head (fine-tuning) --------------------------------------
 * The readout of the reference's fine-tuning models after the pooling
 * (models/ginet_finetune.py:95-127,145-147, models/gcn_finetune.py:131-164)
 * with finetune.py:71-77's criterion, as one chain:
 *   a_0 = x [rows, dims[0]];  a_l = act_l(a_{l-1} W_l^T + b_l),  l = 1..L
 * W_l [dims[l], dims[l-1]] row-major fp32 as nn.Linear stores it, L <=
 * MOLCLR_TASK_HEAD_MAX_LAYERS, any rows >= 1 and any width in [1,
 * MOLCLR_TASK_HEAD_MAX_DIM] (no multiple-of-4 rule; wider: MOLCLR_ERR_UNSUPPORTED,
 * the row block's activations no longer fit the LDS -- molclr_amd.ops composes
 * such chains from the GEMMs).  Every a_l is written to a[l-1] ([rows, dims[l]], dense):
 * the backward reads them, and the models return a_1 (h) and a_L (pred).
 * Softplus is nn.Softplus() (beta 1, threshold 20); its derivative is
 * recomputed from the saved a_l as -expm1(-a_l).
 * Loss on pred = a_L:
 *   CROSS_ENTROPY  target int64 [rows], dims[L] <= MOLCLR_TASK_HEAD_MAX_CLASSES:
 *       mean_rows(logsumexp(pred) - pred[y]), row max subtracted.  A label
 *       outside [0, dims[L]) is never used as an index: it sets
 *       MOLCLR_STATUS_LABEL_RANGE in *status (nullable) and its row's loss and
 *       gradient are NaN.
 *   MSE / L1       target float [rows, dims[L]], mean over all elements
 *       (L1's gradient is sign(diff), 0 at diff == 0).
 * The scalar goes to *loss_out.  The mean is a fixed-order sum (no floating
 * point atomics anywhere): results are bit-identical from run to run.  `sync`
 * is an int32 device word that is 0 on entry and 0 again when the forward
 * has finished (the ticket of the workgroup that reduces the rows); calls that
 * may overlap need their own word.
 * Forward: one launch.  Backward: two launches -- the deltas of every layer
 * down to dx (row-blocked; *gloss scales the loss term, dh / dpred are optional
 * extra gradients into a_1 / a_L, gloss NULL = no loss term), then dW_l =
 * delta_l^T a_{l-1} and db_l = sum_rows delta_l of all layers in one grid, each
 * element summed over the rows in ascending order; accumulate[l] adds into
 * dweight[l] / dbias[l] instead of overwriting.  A NULL dx, dweight[l] or
 * dbias[l] is not computed.  Both directions take a workspace of
 * molclr_task_head_workspace_bytes (0 for an invalid descriptor). */
#define MOLCLR_TASK_HEAD_MAX_LAYERS 10
#define MOLCLR_TASK_HEAD_MAX_CLASSES 16
#define MOLCLR_TASK_HEAD_MAX_DIM 2044
#define MOLCLR_STATUS_LABEL_RANGE 16 /* status bit: class label outside [0, C) */
enum { MOLCLR_ACT_NONE = 0, MOLCLR_ACT_RELU = 1, MOLCLR_ACT_SOFTPLUS = 2 };
enum {
  MOLCLR_LOSS_NONE = 0,
  MOLCLR_LOSS_CROSS_ENTROPY = 1,
  MOLCLR_LOSS_MSE = 2,
  MOLCLR_LOSS_L1 = 3
};

typedef struct molclr_task_head {
  int32_t num_layers;
  int32_t loss;
  int64_t rows;
  int64_t dims[MOLCLR_TASK_HEAD_MAX_LAYERS + 1];
  int32_t act[MOLCLR_TASK_HEAD_MAX_LAYERS];
  const float* x;
  int64_t ldx;
  const float* weight[MOLCLR_TASK_HEAD_MAX_LAYERS];
  const float* bias[MOLCLR_TASK_HEAD_MAX_LAYERS];
  float* a[MOLCLR_TASK_HEAD_MAX_LAYERS];
  const void* target; /* by loss; NULL for MOLCLR_LOSS_NONE */
  float* loss_out;
  int32_t* status;
  int32_t* sync;
} molclr_task_head;

typedef struct molclr_task_head_grads {
  const float* gloss; /* device scalar, nullable */
  const float* dh;    /* [rows, dims[1]], nullable */
  const float* dpred; /* [rows, dims[L]], nullable */
  float* dx;          /* [rows, lddx], nullable */
  int64_t lddx;
  float* dweight[MOLCLR_TASK_HEAD_MAX_LAYERS];
  float* dbias[MOLCLR_TASK_HEAD_MAX_LAYERS];
  int32_t accumulate[MOLCLR_TASK_HEAD_MAX_LAYERS];
} molclr_task_head_grads;

size_t molclr_task_head_workspace_bytes(const molclr_task_head* head);
int molclr_task_head_fwd(const molclr_task_head* head, void* workspace, size_t workspace_bytes,
                         molclr_stream_t stream);
int molclr_task_head_bwd(const molclr_task_head* head, const molclr_task_head_grads* grads,
                         void* workspace, size_t workspace_bytes, molclr_stream_t stream);

/* ---- Motif readout (fine-tuning, motif model) --------------------------------
 * models/ginet_finetune_mp.py:158-160: PyG 1.6.3's GlobalAttention(gate_nn =
 * Linear(F, 1)) over cat(motif_embedding(clique_idx), h) by mol_idx.  B
 * molecules; the T motif items are clique_idx int64 [T] with mol_ptr int32
 * [B + 1] (0 = p_0 <= ... <= p_B = T), so the rows of segment b are
 * E[clique_idx[i]] for i in [p_b, p_{b+1}) in order, then h[b] LAST (the
 * reference appends the h rows after all motif rows).  gate g = x.w + c,
 * alpha = exp(g - max_seg g) / sum_seg exp(g - max), a[b] = sum alpha_i x_i in
 * that row order (PyG's + 1e-16 on a sum that is at least 1 vanishes in fp32
 * and is omitted).  h, a [B, F], E [num_motifs, F], w [F], c [1] dense fp32;
 * alpha [T + B]: the items' weights, then the h rows' -- saved for the backward.
 * Any F >= 1 (16-byte accesses when F % 4 == 0 and the pointers allow), any
 * number of items per molecule (none: a[b] = h[b]), repeated motif ids.
 * A clique_idx outside [0, num_motifs) or a mol_ptr that breaks the rule
 * above is never used as an index: it sets MOLCLR_STATUS_MOTIF_RANGE in
 * *status (nullable) and that molecule's a row (and gradients) are NaN.
 * Forward: one launch, one workgroup per molecule.  Backward: two launches --
 * per molecule s_i = da.x_i, t = sum alpha_i s_i, dgate_i = alpha_i (s_i - t)
 * (computed as alpha_i da.(x_i - a[b]) from the forward's a: no cancellation),
 * dh[b] = alpha_h da[b] + dgate_h w; then one grid for dE[m] = sum over the
 * items of motif m of (alpha_i da[mol(i)] + dgate_i w), dw = sum dgate_i x_i
 * and dc = sum dgate_i.  dE needs the items grouped by motif id: sorted_idx
 * (clique_idx in ascending order) and order (the item at each sorted position)
 * of a STABLE sort, so every sum runs in ascending item order (dw and dc:
 * within a molecule, then over the molecules).  No floating-point atomics:
 * results are bit-identical from run to run.  acc_* add into dE / dweight /
 * dbias instead of overwriting; without acc_dE the rows of E that no item uses
 * are zeroed.  A NULL dh, dE, dweight or dbias is not computed.  The backward
 * takes a workspace of molclr_motif_pool_workspace_bytes (0 for invalid
 * sizes); nothing allocates or synchronises. */
#define MOLCLR_STATUS_MOTIF_RANGE 32 /* status bit: motif id / mol_ptr out of range */
size_t molclr_motif_pool_workspace_bytes(int64_t B, int64_t T, int64_t F);
int molclr_motif_pool_fwd(const float* h, const float* E, const int64_t* clique_idx,
                          const int32_t* mol_ptr, const float* gate_weight, const float* gate_bias,
                          int64_t B, int64_t T, int64_t F, int64_t num_motifs, float* a,
                          float* alpha, int32_t* status, molclr_stream_t stream);
int molclr_motif_pool_bwd(const float* da, const float* h, const float* E,
                          const int64_t* clique_idx, const int32_t* mol_ptr,
                          const int64_t* sorted_idx, const int64_t* order, const float* gate_weight,
                          const float* a, const float* alpha, int64_t B, int64_t T, int64_t F, int64_t num_motifs,
                          float* dh, float* dE, float* dweight, float* dbias, int acc_dE,
                          int acc_dweight, int acc_dbias, void* workspace, size_t workspace_bytes,
                          molclr_stream_t stream);
/* Device-sized form, for a captured step whose item count changes from replay
 * to replay: the same kernels over an item CAPACITY T_cap in place of T.
 * T_cap sizes every buffer, grid and the workspace
 * (molclr_motif_pool_cap_workspace_bytes); alpha is [T_cap + B] with the h
 * rows' weights at T_cap + b; clique_idx, sorted_idx and order hold T_cap
 * entries.  The item count is read on the device as mol_ptr[B]: the rule is
 * 0 = p_0 <= ... <= p_B <= T_cap, and a mol_ptr that breaks it sets
 * MOLCLR_STATUS_MOTIF_RANGE and gives NaN rows as above.  Items [p_B, T_cap)
 * are padding of any value: never an index, no contribution to a, dh, dE,
 * dweight or dbias wherever the stable sort of all T_cap ids put them; a table
 * row that only padding names is 0 without acc_dE and untouched with it.
 * Arithmetic and summation orders are the host-sized form's: on the same items
 * both give bit-identical results.  molclr_stage_motif fills the buffers. */
size_t molclr_motif_pool_cap_workspace_bytes(int64_t B, int64_t T_cap, int64_t F);
int molclr_motif_pool_fwd_cap(const float* h, const float* E, const int64_t* clique_idx,
                              const int32_t* mol_ptr, const float* gate_weight,
                              const float* gate_bias, int64_t B, int64_t T_cap, int64_t F,
                              int64_t num_motifs, float* a, float* alpha, int32_t* status,
                              molclr_stream_t stream);
int molclr_motif_pool_bwd_cap(const float* da, const float* h, const float* E,
                              const int64_t* clique_idx, const int32_t* mol_ptr,
                              const int64_t* sorted_idx, const int64_t* order,
                              const float* gate_weight, const float* a, const float* alpha,
                              int64_t B, int64_t T_cap, int64_t F, int64_t num_motifs, float* dh,
                              float* dE, float* dweight, float* dbias, int acc_dE, int acc_dweight,
                              int acc_dbias, void* workspace, size_t workspace_bytes,
                              molclr_stream_t stream);

/* ---- Captured fine-tuning step (molclr_amd/finetune_step.py) -----------------
 * The fine-tuning loops (finetune.py:89-102 a training batch, finetune.py:259-317
 * an evaluation pass) replayed from HIP graphs over one staged segment.
 *   molclr_stage_task (outside the captured region; one launch):
 *     molclr_stage_segments of ONE segment -- same buffers, same refusals --
 *     that also copies the batch's targets to target_dst, the fixed buffer the
 *     graph's task head reads: int64 labels [target_rows] (target_is_float 0,
 *     target_cols 1) or fp32 values [target_rows, target_cols].  target_rows
 *     must be dst->num_graphs.
 *   molclr_task_step_tail (the training graph's closing launch): advances the
 *     step counters of up to two Adam optimizers (either may be NULL; GCN has
 *     a base and a pred_lin group), copies the loss scalar and ORs the batch's
 *     status word into the sticky word, as molclr_step_tail.
 *   molclr_eval_tail (the evaluation graph's closing launch; one workgroup):
 *     with n = *cursor, copies pred [B, C] to pred_all[n : n + B] and the
 *     staged targets (target_row_words 4-byte words per row: 2 for int64
 *     labels, C for fp32 values) to target_all[n : n + B], adds
 *     (double)*loss * B to *loss_acc, ORs *status_src (nullable) into
 *     *status_acc and sets *cursor = n + B.  If n + B > capacity (rows of
 *     pred_all / target_all) nothing is stored, the cursor and the sum stay,
 *     and MOLCLR_STATUS_EVAL_OVERFLOW is set in *status_acc.
 *   molclr_stage_motif (outside the captured region; one launch): the motif
 *     model's items -- mol_idx int64 [T + B] (the molecule of every item,
 *     ascending, then 0 .. B - 1) and clique_idx int64 [T] -- into the buffers
 *     molclr_motif_pool_*_cap read: clique [T_cap] (the ids, then
 *     MOLCLR_MOTIF_PAD, which no table holds), mol_ptr int32 [B + 1] (the
 *     first item of every molecule, by binary search), sorted_idx / order
 *     [T_cap] (the stable sort of clique by id, padding last; a rank sort, no
 *     scratch memory).  T > T_cap, a mol_idx[:T] that does not ascend and a
 *     mol_idx value outside [0, B) set MOLCLR_STATUS_ITEM_OVERFLOW, _ORDER and
 *     _MOL in *status (nullable; ORed) and make every mol_ptr entry -1, which
 *     the pool answers with MOLCLR_STATUS_MOTIF_RANGE and NaN rows; nothing is
 *     stored outside the buffers. */
#define MOLCLR_STATUS_EVAL_OVERFLOW 64 /* status bit: evaluation rows past the capacity */
#define MOLCLR_STATUS_ITEM_OVERFLOW 128 /* status bit: more motif items than the capacity */
#define MOLCLR_STATUS_ITEM_ORDER 256    /* status bit: mol_idx[:T] not ascending */
#define MOLCLR_STATUS_ITEM_MOL 512      /* status bit: mol_idx outside [0, B) */
#define MOLCLR_MOTIF_PAD INT64_MAX      /* a padding item's id */
int molclr_stage_motif(const int64_t* mol_idx, const int64_t* clique_idx, int64_t T, int64_t B,
                       int64_t T_cap, int64_t* clique, int32_t* mol_ptr, int64_t* sorted_idx,
                       int64_t* order, int32_t* status, molclr_stream_t stream);
int molclr_stage_task(const molclr_stage_source* src, const molclr_graph_staged_segment* dst,
                      int64_t* x_all, int64_t num_nodes_cap, int64_t num_edges_cap,
                      int64_t* counts, const void* target_src, void* target_dst,
                      int64_t target_rows, int64_t target_cols, int target_is_float,
                      molclr_stream_t stream);
int molclr_task_step_tail(int32_t* step_a, int32_t* step_b, const float* loss_src,
                          float* loss_dst, const int32_t* status_src, int32_t* status_acc,
                          molclr_stream_t stream);
int molclr_eval_tail(const float* pred, const void* target, int64_t B, int64_t C,
                     int64_t target_row_words, const float* loss, float* pred_all,
                     void* target_all, int64_t capacity, int64_t* cursor, double* loss_acc,
                     const int32_t* status_src, int32_t* status_acc, molclr_stream_t stream);

/* ---- Device collate of labelled molecules (molclr_amd/task_store.py) ----------
 * The fine-tuning counterpart of molclr_mask_views: MolTestDataset's molecules
 * (dataset_test.py:114-169) resident in the molclr_mask_views store, featurised
 * once, next to a target table -- int64 [G] class labels (target_is_float 0,
 * target_cols 1) or fp32 [G, target_cols] -- and, for the motif model, the
 * assignments as a CSR (motif_ptr int64 [G + 1], motif_ids int64).  mol_ids
 * int64 [batch_size] on the device picks the batch, in any order, repeats
 * allowed.  Every entry point runs on the given stream, allocates nothing and
 * never synchronises; x / edge_attr buffers must be 16-byte aligned (their
 * rows move as one 16-byte record).
 *   molclr_collate_task (eager; a scan launch and a gather launch): the Batch
 *     fields of Batch.from_data_list -- x_out [num_nodes, 2], edge_index_out
 *     [2, num_edges] (local indices shifted by the molecule's first row),
 *     edge_attr_out [num_edges, 2], batch_out [num_nodes], ptr_out
 *     [batch_size + 1] -- molecule k's rows before molecule k + 1's, every
 *     molecule's directed edges in store order, no bond dropped (num_edges =
 *     2 Σ bonds); target_out int64 [batch_size] or fp32 [batch_size,
 *     target_cols].  num_nodes / num_edges come from the host.  status [1] i32
 *     (written, not ORed): bit 0 a molecule id out of range (it contributes no
 *     rows, its target row is 0, nothing is read out of bounds), bit 1 the
 *     host's num_nodes / num_edges are not the device's sums (nothing is stored
 *     past them), bit 2 a stored edge index outside its molecule (clamped).
 *   molclr_stage_task_ids (outside the captured region): the same gather into
 *     the buffers molclr_stage_task fills -- x_all (rows [num_nodes,
 *     num_nodes_cap) zeroed), the segment's edge_index (rows at stride
 *     edge_cap), edge_attr and batch, counts = (num_nodes, num_edges),
 *     target_dst.  batch_size must be dst->num_graphs.  Host sizes beyond the
 *     capacities are refused before any launch with MOLCLR_ERR_ARG, by
 *     molclr_stage_task's own plan and messages.  Device sums that disagree
 *     with the host's set status bit 1 and counts = (0, 0); nothing is stored
 *     past the capacities.  *status is written; the caller ORs it into its
 *     sticky word.
 *   molclr_motif_items (eager): mol_idx int64 [T + batch_size] and clique_idx
 *     int64 [T] of the batch -- molecule 0's motif ids, molecule 1's, ..., each
 *     with its position in the batch, then 0 .. batch_size - 1
 *     (finetune.py:202-210).  T comes from the host.  status [1] (written): bit
 *     0 a molecule id out of range (no items), bit 1 T is not the device's sum;
 *     either makes the trailing batch_size rows of mol_idx -1.
 *   molclr_stage_motif_ids (outside the captured region): those items, expanded
 *     into the workspace, through molclr_stage_motif itself -- same buffers,
 *     same stable sort, same status bits ORed into *status (T > T_cap:
 *     MOLCLR_STATUS_ITEM_OVERFLOW; a refused id or a T that is not the device's
 *     sum: MOLCLR_STATUS_ITEM_MOL, by the -1 rows above). */
size_t molclr_collate_task_workspace_bytes(int64_t batch_size);
int molclr_collate_task(const int64_t* store_x, const int64_t* store_atom_ptr,
                        const int64_t* store_edge_index, const int64_t* store_edge_attr,
                        const int64_t* store_bond_ptr, int64_t store_mols, int64_t store_edges,
                        const int64_t* mol_ids, int64_t batch_size, const void* target_table,
                        int64_t target_cols, int target_is_float, int64_t* x_out,
                        int64_t* edge_index_out, int64_t* edge_attr_out, int64_t* batch_out,
                        int64_t* ptr_out, void* target_out, int64_t num_nodes, int64_t num_edges,
                        int32_t* status, void* workspace, size_t workspace_bytes,
                        molclr_stream_t stream);
/* workspace: molclr_collate_task_workspace_bytes(batch_size) */
int molclr_stage_task_ids(const int64_t* store_x, const int64_t* store_atom_ptr,
                          const int64_t* store_edge_index, const int64_t* store_edge_attr,
                          const int64_t* store_bond_ptr, int64_t store_mols, int64_t store_edges,
                          const int64_t* mol_ids, int64_t batch_size, const void* target_table,
                          int64_t target_cols, int target_is_float, int64_t num_nodes,
                          int64_t num_edges, const molclr_graph_staged_segment* dst,
                          int64_t* x_all, int64_t num_nodes_cap, int64_t num_edges_cap,
                          int64_t* counts, void* target_dst, int32_t* status, void* workspace,
                          size_t workspace_bytes, molclr_stream_t stream);
size_t molclr_motif_items_workspace_bytes(int64_t batch_size);
int molclr_motif_items(const int64_t* motif_ptr, const int64_t* motif_ids, int64_t store_mols,
                       const int64_t* mol_ids, int64_t batch_size, int64_t T, int64_t* mol_idx,
                       int64_t* clique_idx, int32_t* status, void* workspace,
                       size_t workspace_bytes, molclr_stream_t stream);
size_t molclr_stage_motif_ids_workspace_bytes(int64_t batch_size, int64_t T_cap);
int molclr_stage_motif_ids(const int64_t* motif_ptr, const int64_t* motif_ids, int64_t store_mols,
                           const int64_t* mol_ids, int64_t batch_size, int64_t T, int64_t T_cap,
                           int64_t* clique, int32_t* mol_ptr, int64_t* sorted_idx, int64_t* order,
                           int32_t* status, void* workspace, size_t workspace_bytes,
                           molclr_stream_t stream);

/* ---- Retrieval: exact top-k inner-product search (no reference counterpart;
 * the nearest-neighbour analysis of the MolCLR paper) -----------------------
 * For every query row i of q [nq, C] (fp32, row stride ldq) the k best rows
 * of db [n, C] (fp32, or bf16 with db_is_bf16 != 0; row stride lddb), without
 * an [nq, n] score matrix in memory: the database is read once per block of
 * 32 queries and k candidates per query stay on chip.
 *   Score: score(i, j) = sum_c q[i][c] * db[j][c], accumulated in fp32 (bf16
 *     values widened exactly).  The summation order of a (query, row) pair
 *     depends on C alone -- not on n, nq, k, idx_base, the pair's position or
 *     the grid -- so the top-k of a sharded database merges exactly.
 *   Order: higher score first, equal scores by lower index; -0.0 equals +0.0
 *     (reported as +0.0); a NaN score ranks, and is reported, as -inf.
 *   Output: row i of scores / idx [nq, k] holds the k best rows under that
 *     order, sorted by it; indices are j + idx_base.  Row j is skipped for
 *     query i when exclude != NULL and exclude[i] == j + idx_base (the query
 *     is itself in the library).  With fewer than k rows left the remaining
 *     entries are score = -inf, idx = -1.
 *   Limits: 1 <= k <= 64; C % 4 == 0, 4 <= C <= 2048; ldq, lddb >= C with q,
 *     db and every row 16-byte aligned; n, nq >= 0 (0 is a valid call).  All
 *     row offsets are 64-bit.  A refused argument, a workspace below
 *     molclr_topk_dot_workspace_bytes included, is MOLCLR_ERR_ARG before any
 *     HIP call.  The workspace size is non-decreasing in nq and k.
 *   No floating-point atomics: results are bit-reproducible run to run. */
size_t molclr_topk_dot_workspace_bytes(int64_t nq, int64_t n, int64_t C, int k);
int molclr_topk_dot(const float* q, int64_t ldq, const void* db, int64_t lddb, int db_is_bf16,
                    int64_t nq, int64_t n, int64_t C, int k, const int64_t* exclude,
                    int64_t idx_base, float* scores, int64_t* idx, void* workspace,
                    size_t workspace_bytes, molclr_stream_t stream);

/* ---- Benchmark instrumentation (no reference counterpart) -------------------
 * Opt-in kernel timer.  While a kind is enabled, its launches go through
 * hipExtLaunchKernelGGL with a start/stop event pair recorded by the dispatch
 * itself, so each sample is the kernel's own execution window (the figure
 * rocprofv3 --kernel-trace reports).  Kinds (a bit mask): 1 = k_gine_agg_fwd,
 * 2 = every kernel of molclr_gemm_f32 (main GEMM + split-K reduce), 4 = the
 * NT-Xent similarity kernels, 8 = k_gcn_agg_fwd. */
#define MOLCLR_KTIMER_GINE_AGG 1
#define MOLCLR_KTIMER_GEMM 2
#define MOLCLR_KTIMER_NTXENT 4 /* k_ntxent_fwd_partial / k_ntxent_bwd_partial */
#define MOLCLR_KTIMER_GCN_AGG 8
int molclr_ktimer_start(int kinds_mask);
/* Waits for the recorded launches of `kind`, returns their summed duration
 * and count, and forgets them. */
int molclr_ktimer_read(int kind, double* total_ms, int64_t* launches);
/* Disables timing and discards unread samples. */
int molclr_ktimer_stop(void);

#ifdef __cplusplus
}
#endif
#endif /* MOLCLR_H_ */
