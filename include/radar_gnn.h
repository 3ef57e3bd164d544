/*
 * radar_gnn.h -- C ABI of the MI355X-native radar GNN hot path (libradargnn.so).
 *
 * The library replaces the implicit numpy / ATen / PyG kernels of the
 * reference's per-frame path (UditBhaskar19/GRAPH_NEURAL_NETWORK_FOR_RADAR_PERCEPTION v2):
 *   graph build      modules/compute_features/graph_features.py:11-164
 *   model forward    modules/neural_net/gnn/gnn_detector.py:141-201,
 *                    modules/neural_net/gnn/gnn_blocks.py:19-389,
 *                    modules/neural_net/common.py:185-267
 * Each entry point names the reference interface it replaces.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name ends in _host;
 *  - buffers are owned by the caller (the library allocates nothing that
 *    outlives a call; scratch comes from a caller workspace sized by the
 *    matching *_workspace_size function);
 *  - work is enqueued asynchronously on `stream` (a hipStream_t); no entry point
 *    synchronises the host, so a caller may capture them in a hipGraph;
 *  - a batch of radar frames is a disjoint union: nodes of frame f are the rows
 *    [frame_ptr[f], frame_ptr[f+1]) of every node array (frame_ptr: int32[B+1]);
 *  - the adjacency is CSR (row_ptr int32[N+1], col int32[E]) with rows and
 *    columns ascending: position p of row i is edge_index[:, p] = (i, col[p]) of
 *    the reference's np.where order (graph_features.py:79);
 *  - return value 0 = success; otherwise an RG_ERR_* code and rg_last_error()
 *    describes it (the Python layer raises RuntimeError with that text).
 */
#ifndef RADAR_GNN_H
#define RADAR_GNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RG_OK 0
#define RG_ERR_ARG 1
#define RG_ERR_HIP 2
#define RG_ERR_UNSUPPORTED 3

/* element types */
#define RG_F32 0
#define RG_BF16 1
#define RG_F16 6 /* IEEE binary16: the fp16 path (BASELINE config 5) of the 16-bit kernels */
#define RG_F32X3 7 /* rg_mlp_chain: float32 arithmetic on the bf16 matrix cores (every product
                      from exact three-term bf16 splits, f32 accumulation); layers packed
                      RG_BF16 | RG_PACK_X3; training tapes allowed */
/* packed-weight formats of rg_pack_linear: RG_F32 / RG_BF16 for rg_mlp_chain, and
 * the two 32x32x16 bf16 formats of rg_mlp_chain_fast (first layer / chained layers) */
#define RG_PACK_FAST_IN 2
#define RG_PACK_FAST_CHAIN 3
#define RG_PACK_FAST_UPD 4 /* update layer of rg_conv_layer_fused: cat(x, aggregate) */
/* float32 32x32x2 fragments of the register-resident f32 kernels (rg_mlp_chain_f32,
 * rg_conv_layer_f32): fragment (m, s4) = 1 KiB at byte (m * K/8 + s4) * 1024, lane l's
 * 16 B = W[32m + (l & 31)][8 s4 + 4 (l >> 5) + u], u = 0..3 (K padded to 8, N to 32),
 * then the bias in accumulator order [m][h][16] (entry 4g + t = b[32m + 8g + 4h + t]) */
#define RG_PACK_F32_FAST 5
/* OR-ed into a RG_PACK_FAST_* format for a layer followed by channel_normalization:
 * the rows of W and b are shifted to zero mean over the outputs (W - 1 mean_o(W),
 * b - mean(b)).  The normalisation then sees (x - mean) directly -- it is invariant
 * to that shift -- and skips its mean pass.  Mark such layers RG_LAYER_CENTERED. */
#define RG_PACK_CENTERED 0x100
/* OR-ed into RG_F32: `weight` holds the TRANSPOSE of the packed layer, i.e. a row-major
 * [in_dim][out_dim] matrix (the backward data GEMM dX = dZ W packs W^T this way) */
#define RG_PACK_TRANSPOSE 0x200
/* OR-ed into a RG_PACK_FAST_* format: the exact three-term bf16 split of every weight,
 * w = w0 + w1 + w2 (w0 = bf16(w), w1 = bf16(w - w0), w2 = bf16(w - w0 - w1), each residue
 * exact in float32), as three planes of that format back to back, then the float32 bias in
 * accumulator order -- the operand format of the float32 kernels on bf16 matrix cores
 * (rg_conv_layer_x3) */
#define RG_PACK_X3 0x400
/* OR-ed into a RG_PACK_FAST_* format: IEEE fp16 fragments instead of bf16 (round to nearest
 * even); mark such layers RG_LAYER_F16 -- the 16-bit kernels then take fp16 operands */
#define RG_PACK_F16 0x800
/* OR-ed into a RG_PACK_FAST_* format (with RG_PACK_CENTERED as RG_PACK_X3 takes it): the
 * two-term IEEE fp16 split of every weight times a power of two 2^s per layer,
 * w 2^s = w0 + w1 + r (w0 = fp16(w 2^s), w1 = fp16(w 2^s - w0), |r| <= 2^-21 |w| 2^s + 2^-25),
 * as two planes of that format back to back, then the float32 bias times 2^s in accumulator
 * order, then 16 bytes {float 2^-s, float 2^s, int s, 0}.  s is chosen so that the largest
 * |w| of the layer (after centring) times 2^s lies in [2^12, 2^13), within |s| <= 64 (s = 0
 * for an all-zero layer).  The operand format of rg_mlp_chain_x3's three-product scheme: mark
 * such layers RG_LAYER_H2.  Every activation such a chain converts must be below 2^15 in
 * magnitude (fp16 overflows above 65504; the row then comes back non-finite). */
#define RG_PACK_H2 0x1000

/* activations (modules/neural_net/common.py:256-267) */
#define RG_ACT_NONE 0
#define RG_ACT_RELU 1
#define RG_ACT_LEAKY 2
#define RG_ACT_SWISH 3

/* graph modes */
#define RG_GRAPH_KNN 0        /* compute_adjacency_information     graph_features.py:58-84  */
#define RG_GRAPH_RADIUS 1     /* np.where(compute_ball_query(D,eps)) graph_features.py:11-22 */
#define RG_GRAPH_KNN_RADIUS 2 /* compute_adjacency_information_v2  graph_features.py:87-114 */

/* segment reductions (PyG aggr, gnn_blocks.py:57; cluster max gnn_blocks.py:384-387) */
#define RG_REDUCE_SUM 0
#define RG_REDUCE_MEAN 1
#define RG_REDUCE_MAX 2

/* chain input prologues */
#define RG_IN_DENSE 0   /* row r <- in0[r]                                           */
#define RG_IN_CONCAT2 1 /* row r <- cat(in0[r], in1[r])          gnn_blocks.py:108   */
#define RG_IN_GATHER3 2 /* row r <- cat(in0[idx0[r]], in0[idx1[r]], in2[r])
                           = cat(x_i, x_j, e) of MessagePassing.message, gnn_blocks.py:113 */
#define RG_IN_PAIRADD 3 /* row r <- in0[idx0[r]] + in0[idx1[r]]  gnn_blocks.py:297   */
#define RG_IN_PAIRPRE 4 /* rg_mlp_chain_x3 only: layer 0's pre-activation <- in0[idx0[r]] +
                           in0[idx1[r]] + b0, in0 = per-node rows W0 x (layer 0 is linear
                           before its norm, gnn_blocks.py:292-297); layer 0's weights unread */

const char* rg_last_error(void);
int rg_version(void);

/* ---------------------------------------------------------------- graph build */

/* Bytes of scratch rg_build_graph needs. */
size_t rg_build_graph_workspace_size(int n_nodes, int n_frames, int max_frame_nodes, int k,
                                     int mode);

/* Batched compute_adjacency_information (graph_features.py:58-84):
 *   D[i,j] = dx*dx + dy*dy in float32 without FMA (graph_features.py:69-76);
 *   ball_degree[i] = #{j != i : D[i,j] <= eps2}          (:11-22, :78);
 *   kNN: the k+1 smallest (D, j) pairs of each row (all j if k >= N_f),
 *        ties -> lower j (a stable argsort; the reference's default argsort is
 *        unstable, so at exact ties it is implementation-defined) (:25-44);
 *   adjacency = knn | knn^T minus the diagonal (mode KNN), the ball query
 *   (mode RADIUS) or their union (mode KNN_RADIUS);
 *   row_ptr/col = np.where(adjacency) as CSR (:79), global node ids.
 * px, py:        float32[n_nodes]
 * frame_ptr:     int32[n_frames+1] (device)
 * col:           int32[col_capacity]; rg_build_graph fails with RG_ERR_ARG
 *                through *n_edges_out > col_capacity (checked on device: the
 *                overflowing rows are not written and n_edges_out reports the need)
 * n_edges_out:   int32[1] device scalar = E
 */
int rg_build_graph(const float* px, const float* py, const int* frame_ptr, int n_nodes,
                   int n_frames, int max_frame_nodes, int k, float eps2, int mode,
                   int* row_ptr, int* col, long col_capacity, int* ball_degree,
                   int* n_edges_out, void* workspace, size_t workspace_bytes, void* stream);

/* compute_node_features(include_region_confidence=True) (graph_features.py:117-144),
 * cast to float32 as datagen_gnn.py:122 does.  out: float32[n_nodes][6] =
 * (vr, rcs, t_norm, degree/10, range_conf, azimuth_conf). */
int rg_node_features(const float* px, const float* py, const float* vr, const float* rcs,
                     const int64_t* timestamp, const int* ball_degree, const int* frame_ptr,
                     int n_nodes, int n_frames, double min_range, double max_range,
                     double min_azimuth, double max_azimuth, float* out, void* stream);

/* compute_edge_features (graph_features.py:147-164) -> float32[E][7]
 * (dx, dy, dl, dvx, dvy, dv, dt) of every edge src[p] -> dst[p].  With
 * (src, dst) = (edge_index[0], edge_index[1]) this is the reference layout; the
 * message passing passes its destination-major (source, destination) arrays.
 * n_edges_dev (optional device int32) overrides n_edges (then the capacity). */
int rg_edge_features(const float* px, const float* py, const float* vx, const float* vy,
                     const int64_t* timestamp, const int* src, const int* dst,
                     const int* n_edges_dev, long n_edges, float* out, void* stream);

/* The float64 arrays compute_node_features / compute_edge_features themselves return
 * (graph_features.py:144,164: np.stack promotes the float32 columns exactly, while
 * t_norm, degree/10, range_conf and dt are float64 computations), same layouts. */
int rg_node_features_f64(const float* px, const float* py, const float* vr, const float* rcs,
                         const int64_t* timestamp, const int* ball_degree, const int* frame_ptr,
                         int n_nodes, int n_frames, double min_range, double max_range,
                         double min_azimuth, double max_azimuth, double* out, void* stream);
int rg_edge_features_f64(const float* px, const float* py, const float* vx, const float* vy,
                         const int64_t* timestamp, const int* src, const int* dst, long n_edges,
                         double* out, void* stream);

/* rg_edge_features from node kinematics packed once per batch: kin = float4[n_nodes]
 * (px, py, vx, vy) from rg_pack_kinematics (16-B aligned).  Same results, two gathers
 * per edge endpoint instead of five. */
int rg_pack_kinematics(const float* px, const float* py, const float* vx, const float* vy,
                       int n_nodes, void* kin, void* stream);
int rg_edge_features_packed(const void* kin, const int64_t* timestamp, const int* src,
                            const int* dst, const int* n_edges_dev, long n_edges, float* out,
                            void* stream);

/* edge_formation's pairs from a DENSE adjacency (gnn_blocks.py:295-296: torch.nonzero(
 * torch.triu(adj, 1), as_tuple=True), row-major), in two calls so the caller sizes the
 * pair arrays from the count (the one host synchronisation, where torch.nonzero syncs too):
 *   rg_dense_pair_rows: adj = uint8 / bool [n][n] (n <= 46340) -> row_ptr int32[n + 1]
 *     (exclusive scan of each row's entries right of the diagonal), n_pairs int32[1];
 *     workspace O(n);
 *   rg_dense_pair_emit: pair_src / pair_dst int32[n_pairs], rows in order, columns
 *     ascending.
 * Any nonzero byte of adj is an entry.  At n = 0: row_ptr[0] = 0, *n_pairs = 0, and
 * rg_dense_pair_emit writes nothing. */
size_t rg_dense_pair_rows_workspace_size(int n_nodes);
int rg_dense_pair_rows(const void* adj, int n_nodes, int* row_ptr, int* n_pairs, void* workspace,
                       size_t workspace_bytes, void* stream);
int rg_dense_pair_emit(const void* adj, int n_nodes, const int* row_ptr, int* pair_src,
                       int* pair_dst, void* stream);
/* out[r][0..w) = x[idx0[r]] + x[idx1[r]] in float32 (edge_formation's x[i] + x[j],
 * gnn_blocks.py:297); rows of x are ldx floats apart, rows of out ld_out (>= w) apart, and
 * the columns [w, ld_out) of out are left alone. */
int rg_pair_add_rows_f32(const float* x, int ldx, int w, const int* idx0, const int* idx1,
                         long rows, float* out, int ld_out, void* stream);

/* Undirected link pairs of edge_formation (gnn_blocks.py:295-296):
 * nonzero(triu(adj,1)) row-major == CSR positions with col > row.
 * pair_ptr int32[n_nodes+1]; pair_src/pair_dst int32[pair_capacity]; n_pairs int32[1].
 * pair_ptr and *n_pairs are always the true offsets and count.  When *n_pairs exceeds
 * pair_capacity, a row whose last pair would lie past the capacity is skipped whole
 * (pair_ptr[row + 1] > pair_capacity): nothing at or past pair_capacity is written, and the
 * entries of the skipped rows are left alone.  Columns ascend within a row of the CSR. */
size_t rg_link_pairs_workspace_size(int n_nodes);
int rg_link_pairs(const int* row_ptr, const int* col, int n_nodes, int* pair_ptr, int* pair_src,
                  int* pair_dst, long pair_capacity, int* n_pairs, void* workspace,
                  size_t workspace_bytes, void* stream);

/* Link pairs of an arbitrary edge_index (int64[2][E], reference order): the
 * positions with edge_index[0] < edge_index[1], in edge order; equals
 * nonzero(triu(adj,1)) when edge_index = np.where(adj) (graph_features.py:79).
 * pair_src / pair_dst int32[*n_pairs] (at most n_edges; nothing past *n_pairs is written);
 * n_pairs int32[1], written at n_edges = 0 too.  The endpoints are only compared, so any
 * int64 values do; the pairs hold their low 32 bits. */
size_t rg_pairs_from_edge_index_workspace_size(long n_edges);
int rg_pairs_from_edge_index(const int64_t* edge_index, long n_edges, int* pair_src, int* pair_dst,
                             int* n_pairs, void* workspace, size_t workspace_bytes, void* stream);

/* out[p] = row of CSR position p (edge_index[0]; destination of a dst-major edge).
 * out int32[row_ptr[n_rows]]: positions from row_ptr[n_rows] on belong to no row and are
 * left alone. */
int rg_csr_rows(const int* row_ptr, int n_rows, int* out, void* stream);

/* Capacity guard for a graph built by rg_build_graph into a capacity the host has not
 * checked (radius graphs without a host sync, graph_features.py:build_graph_batch):
 * need_out[0] = the true edge count (int32 in device memory, or in pinned host memory -- the
 * kernel stores it directly, no copy launch); if it exceeds capacity, row_ptr is cut at a
 * row boundary (the rows rg_build_graph left unwritten become empty) and *n_edges_dev =
 * that boundary, so every consumer stays in bounds.  The host
 * reads need_out later (no sync on the launch path) and treats the step as invalid when
 * need_out[0] > capacity.  (The cut is at the last boundary <= capacity / 2: a cut graph is
 * not symmetric, and the link-pair arrays hold capacity / 2 + 1 pairs.) */
int rg_csr_clamp(int* row_ptr, int n_rows, int* n_edges_dev, long capacity, int* need_out,
                 void* stream);

/* Destination-major CSR of an arbitrary edge_index (int64[2][E], reference order):
 * dst_ptr int32[n_nodes+1]; perm int32[E] (dst-major position -> reference
 * position), ordered by (dst, src, reference position); src_sorted int32[E].
 * An edge with an endpoint outside [0, n_nodes) is not an edge of the graph: it is dropped,
 * and dst_ptr[n_nodes] -- the number of edges kept -- reports it by falling short of E.  The
 * kept edges are exact; the E - dst_ptr[n_nodes] positions past them in perm and src_sorted
 * are written 0.  The caller compares dst_ptr[n_nodes] with E before it trusts the graph
 * (engine.DeviceGraph.from_edge_index raises IndexError). */
size_t rg_csr_by_dst_workspace_size(int n_nodes, long n_edges);
int rg_csr_by_dst(const int64_t* edge_index, long n_edges, int n_nodes, int* dst_ptr, int* perm,
                  int* src_sorted, void* workspace, size_t workspace_bytes, void* stream);

/* Dense views for the numpy-level drop-in compute_adjacency_information of ONE
 * frame: adj uint8[N][N] from the CSR and dist float32[N][N] (either may be NULL). */
int rg_dense_adjacency(const float* px, const float* py, const int* row_ptr, const int* col,
                       int n_nodes, uint8_t* adj, float* dist, void* stream);

/* out[r] = (int64) in[r], r < n (edge_index boundary: datagen_gnn.py:123 int64) */
int rg_i32_to_i64(const int* in, long n, int64_t* out, void* stream);

/* out[r][:] = in[idx[r]][:] for float32 rows of width w: in and out are dense (rows w
 * floats apart), out float32[rows][w] */
int rg_gather_rows_f32(const float* in, const int* idx, long rows, int w, float* out,
                       void* stream);

/* --------------------------------------------------------- dense MLP chains */

/* Bytes of one packed Linear(in_dim -> out_dim) in `dtype`. */
size_t rg_packed_linear_bytes(int in_dim, int out_dim, int dtype);

/* Pack a torch nn.Linear (weight float32 [out_dim][in_dim] row-major, bias
 * float32[out_dim] or NULL; device) into the MFMA fragment order the chain
 * kernels read, zero padded, followed by the float32 bias: in plain order padded to a
 * multiple of 16 for RG_F32 and RG_BF16 (32 with RG_PACK_X3), in 32x32 accumulator order
 * padded to a multiple of 32 for RG_PACK_F32_FAST and the RG_PACK_FAST_* formats.  An
 * RG_PACK_H2 image ends with its 16-byte scale trailer. */
int rg_pack_linear(const float* weight, const float* bias, int in_dim, int out_dim, int dtype,
                   void* packed, void* stream);

/* Many float32 packs in ONE launch (the training step re-packs every layer's images after
 * each optimizer step: `optimizer.step()` at training.py:80 changes every nn.Linear).  Each
 * job is what rg_pack_linear(weight, bias, in_dim, out_dim, fmt | (transpose ?
 * RG_PACK_TRANSPOSE : 0), packed) writes, for fmt RG_F32 or RG_PACK_F32_FAST.  jobs: a
 * DEVICE array of n_jobs entries (built once; the weights are read at launch time). */
typedef struct rg_pack_job {
  const float* weight;  /* [out][in] ([in][out] with transpose) */
  const float* bias;    /* [out] or NULL */
  void* packed;         /* rg_packed_linear_bytes(in_dim, out_dim, fmt) bytes */
  int in_dim, out_dim, fmt, transpose;
  int ld;               /* weight's row stride in floats (0: dense rows) */
} rg_pack_job;
int rg_pack_linear_jobs(const rg_pack_job* jobs, int n_jobs, void* stream);
/* rg_pack_linear for RG_F32 / RG_PACK_F32_FAST (| RG_PACK_TRANSPOSE) from a column block of a
 * wider row-major matrix: rows ld floats apart (0: dense).  The training step packs the
 * x_i / x_j / e column blocks of msg0 (gnn_blocks.py:100-101) this way for its factorised
 * message backward. */
int rg_pack_linear_ld(const float* weight, const float* bias, int in_dim, int out_dim, int dtype,
                      int ld, void* packed, void* stream);

/* One ffn_block (common.py:185-205): Linear -> [channel_normalization] -> activation. */
typedef struct rg_layer {
  const void* w_packed;  /* rg_pack_linear output (weights + bias)             */
  const float* norm_mu;  /* channel_normalization.mu  (1,) or NULL (no norm)     */
  const float* norm_std; /* channel_normalization.std (1,)                       */
  int in_dim;
  int out_dim;
  int act;   /* RG_ACT_* */
  int flags; /* RG_LAYER_* */
  /* training forward (rg_mlp_chain, RG_F32 only; NULL for inference): the layer's
   * pre-normalisation output z = x W^T + b and its post-activation output a, both
   * float32 [rows][out_dim] -- the tape rg_ffn_backward / rg_linear_grad read */
  float* save_pre;
  float* save_out;
} rg_layer;

#define RG_LAYER_CENTERED 1 /* w_packed was packed with RG_PACK_CENTERED */
#define RG_LAYER_F16 2      /* w_packed holds fp16 fragments (RG_PACK_F16): the fast chain /
                               fused conv then read and write RG_F16 activations */
#define RG_LAYER_H2 4       /* w_packed was packed with RG_PACK_H2 (rg_mlp_chain_x3: every layer
                               of a chain, or none; rg_conv_layer_x3_for: every image, or none) */

#define RG_MAX_LAYERS 8

/* A chain of up to RG_MAX_LAYERS ffn_blocks over `rows` rows (widths <= 256),
 * fused in one kernel; activations never leave the chip between layers.
 * Covers graph_feature_encoding (gnn_blocks.py:19-42), the message and update
 * MLPs of residual_graph_conv_block (:104-113), the stems and
 * FFN_TaskSpecificHead of every task head (:167-389).
 *   dtype    RG_F32 (f32 MFMA), RG_BF16 / RG_F16 (16-bit operands, f32 accumulation;
 *            RG_F16's layers packed RG_BF16 | RG_PACK_F16), RG_F32X3
 *   in_mode  RG_IN_*: how row r's input vector is formed from in0/in1/in2
 *   in_dtype element type of in0/in1/in2 (RG_F32, RG_BF16 or RG_F16)
 *   rows_dev optional device int32 row count (overrides `rows` when non-NULL;
 *            `rows` is then the capacity used for the grid)
 *   residual optional [rows][out_dim] added after the last layer (:109)
 *   out      [rows][ld_out] in out_dtype
 */
int rg_mlp_chain(int dtype, const rg_layer* layers_host, int n_layers, long rows,
                 const int* rows_dev, int in_mode, int in_dtype, const void* in0, int ld0,
                 int w0, const void* in1, int ld1, int w1, const void* in2, int ld2, int w2,
                 const int* idx0, const int* idx1, const void* residual, int ld_res,
                 int res_dtype, void* out, int ld_out, int out_dtype, void* stream);

/* Register-resident bf16 chain (same semantics as rg_mlp_chain with dtype RG_BF16)
 * for the widths of the shipped architecture: layer 0 packed as RG_PACK_FAST_IN,
 * later layers as RG_PACK_FAST_CHAIN.  Returns RG_ERR_UNSUPPORTED (and launches
 * nothing) when the shape has no compiled instantiation; the caller then uses
 * rg_mlp_chain. */
int rg_mlp_chain_fast(const rg_layer* layers_host, int n_layers, long rows, const int* rows_dev,
                      int in_mode, int in_dtype, const void* in0, int ld0, int w0,
                      const void* in1, int ld1, int w1, const void* in2, int ld2, int w2,
                      const int* idx0, const int* idx1, const void* residual, int ld_res,
                      int res_dtype, void* out, int ld_out, int out_dtype, void* stream);

/* Register-resident float32 chain (same semantics as rg_mlp_chain with dtype RG_F32,
 * exact f32 products on v_mfma_f32_32x32x2_f32) for the widths of the shipped
 * architecture: every layer packed RG_PACK_F32_FAST, no RG_LAYER_CENTERED.  in_mode
 * RG_IN_DENSE (float32 rows; <= 8 features with an un-normalised first layer = the
 * encoders, gnn_blocks.py:19-42) or RG_IN_PAIRADD (edge_formation, gnn_blocks.py:297).
 * Returns RG_ERR_UNSUPPORTED (launching nothing) for shapes without an instantiation;
 * the caller then uses rg_mlp_chain.  Replaces the ffn_block chains of common.py:185-220
 * called from gnn_blocks.py:19-42 and :167-389. */
int rg_mlp_chain_f32(const rg_layer* layers_host, int n_layers, long rows, const int* rows_dev,
                     int in_mode, const float* in0, int ld0, int w0, const int* idx0,
                     const int* idx1, float* out, int ld_out, void* stream);
/* rg_mlp_chain_f32 with every input mode and the training tape: in_mode also
 * RG_IN_GATHER3 (cat(in0[idx0], in0[idx1], in2) with 64-wide parts: the message MLP,
 * gnn_blocks.py:104-113) and RG_IN_CONCAT2 (cat(in0, in1), 64 + 64: the update MLP,
 * :108); optional residual (out = residual + chain, :109); when every layer's save_pre /
 * save_out is set, each layer's z and a rows are written as rg_mlp_chain writes them (the
 * training forward of training.py:66-85); the LAST layer's save_out may be NULL (its
 * activation is the chain output, never read back by the backward).  RG_ERR_UNSUPPORTED (launching nothing) for
 * shapes without an instantiation. */
int rg_mlp_chain_f32_ex(const rg_layer* layers_host, int n_layers, long rows, const int* rows_dev,
                        int in_mode, const float* in0, int ld0, int w0, const float* in1, int ld1,
                        int w1, const float* in2, int ld2, int w2, const int* idx0,
                        const int* idx1, const float* residual, int ld_res, float* out,
                        int ld_out, void* stream);

/* The same float32 chains on the bf16 matrix cores: every product formed from the exact
 * three-term bf16 splits of both operands (RG_PACK_X3, see rg_conv_layer_x3), f32
 * accumulation -- float32 accuracy at 2.7x the f32 MFMA rate.  Layer 0 packed
 * RG_PACK_FAST_IN | RG_PACK_X3, later layers RG_PACK_FAST_CHAIN | RG_PACK_X3.  With
 * RG_PACK_H2 in place of RG_PACK_X3 on every layer (RG_LAYER_H2), each product is formed from
 * two-term fp16 splits in three MFMAs instead of six: float32-class results (the dropped
 * terms are below 2^-21 of a product, under the f32 accumulation error), half the matrix
 * work, inputs and activations limited to |a| < 2^15.  in_mode and the rest as rg_mlp_chain_f32 (dense inputs of <= 8 features
 * with an un-normalised first layer, or widths that are multiples of 16).  Returns
 * RG_ERR_UNSUPPORTED (launching nothing) for shapes without an instantiation, and for the
 * <= 8-input (encoder) shapes also unless the output rows are full width (last out_dim a
 * multiple of 32), ld_out % 4 == 0 and rows * ld_out * 4 <= 0x7ff00000 (their rows are
 * written by buffer stores with 32-bit byte offsets). */
int rg_mlp_chain_x3(const rg_layer* layers_host, int n_layers, long rows, const int* rows_dev,
                    int in_mode, const float* in0, int ld0, int w0, const int* idx0,
                    const int* idx1, float* out, int ld_out, void* stream);

/* The same chain with its output written as SPLIT ROWS: each row of 64 values v keeps its 256
 * bytes, and each aligned 32-byte group of eight values (features 8j .. 8j + 7) holds the
 * eight fp16 heads a0 = fp16(v), 16 bytes, then the eight fp16 residues a1 = fp16(v - a0),
 * 16 bytes -- the two h2 terms of the row, bit for bit what an RG_LAYER_H2 kernel forms when
 * it reads the float32 row (csrc/pack_layout.h: split_row_head / split_row_res).  For rows
 * that several h2 launches read unchanged (the edge rows of a stack of conv layers,
 * rg_conv_layer_x3_split_for): the split is done once by the writer.  RG_ERR_ARG, launching
 * nothing, unless every layer is RG_LAYER_H2, the last out_dim and ld_out are both 64 and
 * out is 16-byte aligned; RG_ERR_UNSUPPORTED for shapes without an instantiation (compiled:
 * the 7 -> 256 -> 128 -> 128 -> 64 edge encoder) and as rg_mlp_chain_x3. */
int rg_mlp_chain_x3_split(const rg_layer* layers_host, int n_layers, long rows, const int* rows_dev,
                          int in_mode, const float* in0, int ld0, int w0, const int* idx0,
                          const int* idx1, void* out, int ld_out, void* stream);

/* One v_mfma_f32_32x32x16_f16 as the RG_PACK_H2 kernels issue it (one wave, zero
 * accumulators): c[m][n] = sum_k a[m][k] b[n][k] with a, b fp16 bit patterns, row-major
 * [32][16], and c float32 [32][32].  The h2 arithmetic rests on fp16 SUBNORMAL operands
 * being honoured, not flushed; the test suite pins that with this entry. */
int rg_h2_mfma_probe(const uint16_t* a, const uint16_t* b, float* c, void* stream);

/* One fused FLOAT32 residual_graph_conv_block (gnn_blocks.py:96-113, the reference
 * precision) for the shipped widths (C = 64, message MLP 192 -> 128 -> 64, update
 * 128 -> 64, channel_normalization + LeakyReLU on every block), aggregation add or mean
 * (the PyG propagate of gnn_blocks.py:57,106).  layers[4], all RG_PACK_F32_FAST:
 *   [0] the per-node projection 64 -> 256: rows 0..127 = W_msg0[:, 0:64] (x_i columns),
 *       rows 128..255 = W_msg0[:, 64:128] (x_j columns); bias = [b_msg0; 0]; no norm / act
 *   [1] W_msg0[:, 128:192] (the edge columns) 64 -> 128, no bias, msg0's norm + act
 *   [2] msg1 128 -> 64 (bias, norm, act)     [3] upd 128 -> 64 on cat(x, agg)
 * seg_ptr / src / dst: destination-major CSR (sources ascending per segment); e rows in
 * that order.  x_out[i] = x[i] + upd(cat(x[i], AGG_p msg(cat(x[i], x[src p], e[p])))),
 * the sum in edge order.  workspace: rg_conv_layer_f32_workspace_size(n_nodes) bytes,
 * no initialisation needed (two launches: projections, which also reset the block
 * counters, then the fused layer); one workspace per stream. */
size_t rg_conv_layer_f32_workspace_size(int n_nodes);
int rg_conv_layer_f32(const rg_layer* layers, int aggr, const float* x, int ldx, const float* e,
                      int lde, const int* seg_ptr, const int* src, const int* dst, int n_nodes,
                      float* x_out, int ld_out, void* workspace, size_t workspace_bytes,
                      void* stream);

/* The same FLOAT32 layer on the bf16 matrix cores: every product of the MLPs is formed
 * from the exact three-term bf16 splits of both operands (six bf16 products of total
 * weight <= 2 per product, f32 accumulation; dropped terms < 2^-23 |a b|), so the layer
 * keeps float32 accuracy at 2.7x the matrix rate of the f32 MFMA path.  Two launches per
 * layer (edge: layers [0], [1] and the in-order segmented sum; node: [2] and next_pq):
 *   layers[3], all RG_PACK_X3: [0] W_msg0[:, 128:192] (edge columns, FAST_IN) with msg0's
 *     norm + act, bias unused; [1] msg1 (FAST_CHAIN); [2] upd on cat(x, agg) (FAST_IN over
 *     the 128 concatenated inputs)
 *   pq        [n_nodes][256] float32: P | Q = W_msg0[:, 0:64] x + b_msg0 | W_msg0[:, 64:128] x,
 *             from rg_conv_proj_x3 (first layer) or the previous layer's pq_out
 *   next_pq   NULL, or the NEXT layer's projection (64 -> 256, FAST_CHAIN | X3, bias
 *             [b_msg0'; 0]): then pq_out [n_nodes][256] receives it from x_out's registers
 *   workspace rg_conv_layer_x3_workspace_size(n_nodes) bytes, block counters ZEROED before
 *             the first call (every completed launch leaves them zero); one per stream.
 * Same results contract as rg_conv_layer_f32 (sum in edge order, mean = sum / max(deg, 1)).
 * With RG_PACK_H2 in place of RG_PACK_X3 on EVERY image (RG_LAYER_H2 on layers[0..2], next_pq
 * and next_we; a mixture is RG_ERR_ARG) the products are two-term fp16 splits, three MFMAs
 * instead of six, as in rg_mlp_chain_x3: float32-class results, every converted value -- x,
 * e, the normalised hidden rows and the AGGREGATE -- limited to |a| < 2^15 (beyond it rows
 * come back non-finite).  Each h2 image carries its own power-of-two scale, and pq rows are
 * then held in the units of the W_e image that accumulates onto them: their writer needs
 * that image (rg_conv_proj_x3_for's we, rg_conv_layer_x3_for's next_we). */
size_t rg_conv_layer_x3_workspace_size(int n_nodes);
int rg_conv_layer_x3(const rg_layer* layers, const rg_layer* next_pq, int aggr, const float* x,
                     int ldx, const float* e, int lde, const float* pq, const int* seg_ptr,
                     const int* src, const int* dst, int n_nodes, float* x_out, int ld_out,
                     float* pq_out, void* workspace, size_t workspace_bytes, void* stream);
/* The same layer with the edge launch's wave table from rg_conv_x3_blocks (built once per
 * graph instead of once per layer): per wave of the one-wave-per-SIMD edge launch S pieces
 * of whole destinations (one per slab of its XCD's node range), equal edge counts.  Same
 * results. */
int rg_conv_layer_x3_blocks(const rg_layer* layers, const rg_layer* next_pq, int aggr,
                            const float* x, int ldx, const float* e, int lde, const float* pq,
                            const int* seg_ptr, const int* src, const int* dst, int n_nodes,
                            float* x_out, int ld_out, float* pq_out, const int* table,
                            void* workspace, size_t workspace_bytes, void* stream);
/* table: rg_conv_x3_blocks_bytes(n_nodes) bytes of device memory -- int32 boundaries of
 * W x S node pieces with equal edge counts in node order (piece q = destinations
 * [table[q], table[q + 1])); wave j of XCD x (W / 8 waves per XCD) takes the pieces
 * (x S + k) W / 8 + j, k = 0 .. S - 1, so the XCD's waves walk its slabs together -- from
 * seg_ptr[n_nodes + 1]. */
size_t rg_conv_x3_blocks_bytes(int n_nodes);
int rg_conv_x3_blocks(const int* seg_ptr, int n_nodes, int* table, void* stream);
/* P | Q of the first layer for dense float32 rows x [n_nodes][ldx >= 64]: pq layer packed
 * RG_PACK_FAST_IN | RG_PACK_X3 (64 -> 256, bias [b_msg0; 0]). */
int rg_conv_proj_x3(const rg_layer* pq, const float* x, int ldx, int n_nodes, float* pq_out,
                    void* stream);
/* The same for either term scheme: we = layers[0] (the W_e image) of the layer that will read
 * pq_out -- required when pq is RG_LAYER_H2 (then also RG_LAYER_H2), ignored (may be NULL)
 * under RG_PACK_X3.  rg_conv_proj_x3 is this call with we = NULL. */
int rg_conv_proj_x3_for(const rg_layer* pq, const rg_layer* we, const float* x, int ldx,
                        int n_nodes, float* pq_out, void* stream);
/* rg_conv_layer_x3 (table NULL) / rg_conv_layer_x3_blocks for either term scheme: next_we =
 * layers[0] of the NEXT layer, the consumer of pq_out -- required with an RG_LAYER_H2
 * next_pq, NULL without next_pq. */
int rg_conv_layer_x3_for(const rg_layer* layers, const rg_layer* next_pq, const rg_layer* next_we,
                         int aggr, const float* x, int ldx, const float* e, int lde,
                         const float* pq, const int* seg_ptr, const int* src, const int* dst,
                         int n_nodes, float* x_out, int ld_out, float* pq_out, const int* table,
                         void* workspace, size_t workspace_bytes, void* stream);
/* rg_conv_layer_x3_for over edge rows given as SPLIT ROWS (rg_mlp_chain_x3_split): the edge
 * launch feeds the loaded halves to its first layer without converting them.  Results are
 * bit-identical to rg_conv_layer_x3_for on the float32 rows.  RG_ERR_ARG, launching nothing,
 * unless the images are RG_LAYER_H2, lde is 64 and e_split is 16-byte aligned;
 * RG_ERR_UNSUPPORTED, launching nothing, where the layer would not run the one-wave edge
 * launch (layers not packed centred, or n_nodes >= 2^22): hand such layers float32 rows. */
int rg_conv_layer_x3_split_for(const rg_layer* layers, const rg_layer* next_pq,
                               const rg_layer* next_we, int aggr, const float* x, int ldx,
                               const void* e_split, int lde, const float* pq, const int* seg_ptr,
                               const int* src, const int* dst, int n_nodes, float* x_out,
                               int ld_out, float* pq_out, const int* table, void* workspace,
                               size_t workspace_bytes, void* stream);

/* The classifier's conv layer over COMPLETE OBJECT GRAPHS, from the object sizes alone
 * (cls_conv_x3.hip).  The graph is the block-diagonal union of complete graphs of
 * compute_edge_index: object o owns the contiguous rows [b_o, b_o + n_o) and the sources of
 * destination i are those rows without i, ascending.  Nothing of E entries is built or read.
 *
 * rg_cls_object_table, once per batch and shared by its layers: from object_size int64[n_obj]
 * on the device (their sum = n_nodes; the host passes n_nodes and n_edges = sum n (n - 1),
 * n_edges < 2^31 or RG_ERR_ARG) the int32 table of rg_cls_object_table_bytes(n_nodes, n_obj)
 * bytes: the destination-major seg_ptr[n_nodes + 1] (degree n_o - 1), every node's object begin
 * and size, and the edge launch's wave table (pieces of whole destinations with equal edge
 * counts).  workspace: rg_cls_object_table_workspace_size(n_obj) bytes.  No host
 * synchronisation; n_nodes == 0 launches nothing. */
size_t rg_cls_object_table_bytes(int n_nodes, int n_obj);
size_t rg_cls_object_table_workspace_size(int n_obj);
int rg_cls_object_table(const int64_t* object_size, int n_obj, int n_nodes, long n_edges,
                        int* table, void* workspace, size_t workspace_bytes, void* stream);
/* One residual conv block of the classifier (classifier/blocks.py:28-85),
 *   x_out[i] = x[i] + leaky(W_u cat(x[i], AGG_{j in object(i), j != i} m_ij) + b_u),
 *   m_ij = leaky(W_1 leaky(P[i] + Q[j]) + b_1),  P | Q = W_pq x + [b_0; 0],
 * in the exact three-term bf16 arithmetic of rg_conv_layer_x3 (float32's range: the classifier's
 * activations are not normalised).  layers[0]: the projection [W_0's x_i columns; its x_j
 * columns] 128 -> 256 with bias [b_0; 0], RG_PACK_FAST_IN | RG_PACK_X3, act = msg0's activation;
 * layers[1]: msg1 128 -> 128, RG_PACK_FAST_CHAIN | RG_PACK_X3; layers[2]: upd 256 -> 128 over
 * cat(x, agg), RG_PACK_FAST_IN | RG_PACK_X3; all un-centred, no norm, RG_ACT_LEAKYRELU.
 * aggr: RG_REDUCE_SUM, _MEAN (by n_o - 1) or _MAX, summed in ascending source order; a node of
 * a one-member object aggregates zeros.  Three launches, no atomics: results are
 * bit-reproducible, and an object's rows do not depend on the other objects of the batch.
 * workspace: rg_cls_conv_layer_x3_workspace_size(n_nodes, n_obj) bytes (no edge count), need
 * not be zeroed.  RG_ERR_UNSUPPORTED, launching nothing, for any other shape, activation, norm
 * or a centred image; RG_ERR_ARG for x == x_out, a short workspace or an RG_LAYER_H2 /
 * RG_LAYER_F16 image; n_nodes <= 0 is a no-op. */
size_t rg_cls_conv_layer_x3_workspace_size(int n_nodes, int n_obj);
int rg_cls_conv_layer_x3(const rg_layer* layers, int aggr, const float* x, int ldx,
                         const int* table, int n_nodes, int n_obj, float* x_out, int ld_out,
                         void* workspace, size_t workspace_bytes, void* stream);
/* The same block for training, edge phase only (the update MLP runs as a taped N-row chain).
 *
 * rg_cls_conv_aggregate_x3: the projection and edge launches of rg_cls_conv_layer_x3 with their
 * results in caller buffers -- pq [n_nodes][256] = P | Q and agg [n_nodes][128] as the update MLP
 * reads it (`mean` divided by n_o - 1, a one-member object's row zero): the bits the fused layer
 * aggregates.  layers[0], layers[1] as above.  aggr RG_REDUCE_SUM or _MEAN (RG_REDUCE_MAX:
 * RG_ERR_UNSUPPORTED -- its backward needs the messages).  workspace:
 * rg_cls_conv_aggregate_x3_workspace_size(n_nodes) bytes.
 *
 * rg_cls_conv_backward_x3 (cls_conv_bwd_x3.hip): from pq and d_agg [n_nodes][128] (row stride
 * ld_dagg, a multiple of 4) it WRITES d_pq [n_nodes][256] = d P | d Q (rows of one-member
 * objects zero) and ADDS d W_1 [128][128], d b_1 [128]:
 *   dm_ij = d_agg[i] leaky'(z1_ij) (mean: times 1 / (n_o - 1)),  dz0_ij = (W_1^T dm_ij) leaky'(z0_ij),
 *   d P[i] = sum_j dz0_ij,  d Q[j] = sum_i dz0_ij,  d W_1 = sum dm_ij h_ij^T,  d b_1 = sum dm_ij
 * with z0, h, z1 recomputed per 32-edge tile from pq: nothing sized by the edge count is read,
 * written or kept.  layers[0]: msg1 as above; layers[1]: a bare Linear of W_1^T (128 -> 128, no
 * bias), RG_PACK_FAST_CHAIN | RG_PACK_X3.  Each d P / d Q row is summed in ascending partner
 * order inside one wave: no atomics, bit-reproducible, an object's rows independent of the rest
 * of the batch.  d W_1 / d b_1: the destination pass runs in chunks of whole destinations of at
 * most 2^17 + max_degree edges whose dm and h rows go to the workspace and through
 * rg_linear_grad.  n_edges = sum n (n - 1) < 2^31 (host); max_degree: an upper bound of
 * n_o - 1 over the objects (n_nodes - 1 always is one, at the price of n_nodes more tape rows per
 * chunk; with a value below the true maximum d W_1 and d b_1 are undefined -- rows of an earlier
 * chunk may be added again -- while d_pq stays right and nothing is written out of bounds).
 * workspace:
 * rg_cls_conv_backward_x3_workspace_size(n_nodes, max_degree) bytes (no edge count), need not be
 * zeroed.  Both: RG_ERR_UNSUPPORTED, launching nothing, for any other shape, activation, norm,
 * aggregation or a centred image; RG_ERR_ARG for an RG_LAYER_H2 / RG_LAYER_F16 image, a short
 * workspace or aliased buffers; n_nodes <= 0 is a no-op. */
size_t rg_cls_conv_aggregate_x3_workspace_size(int n_nodes);
int rg_cls_conv_aggregate_x3(const rg_layer* layers, int aggr, const float* x, int ldx,
                             const int* table, int n_nodes, float* pq, float* agg,
                             void* workspace, size_t workspace_bytes, void* stream);
size_t rg_cls_conv_backward_x3_workspace_size(int n_nodes, int max_degree);
int rg_cls_conv_backward_x3(const rg_layer* layers, int aggr, const float* pq, const float* d_agg,
                            int ld_dagg, const int* table, int n_nodes, long n_edges,
                            int max_degree, float* d_pq, float* d_w1, float* d_b1,
                            void* workspace, size_t workspace_bytes, void* stream);

/* One fused residual_graph_conv_block (gnn_blocks.py:96-113) for the shipped
 * widths (node / edge channels 64, msg MLP 192->128->64, update 128->64, all with
 * channel_normalization), bf16 operands, aggregation add or mean:
 *   x_out[i] = x[i] + upd(cat(x[i], AGG_{p in seg i} msg(cat(x[i], x[src[p]], e[p]))))
 * seg_ptr / src / dst: destination-major CSR (dst[p] = segment of p); e rows in
 * the same order.  msg_layers[0] packed RG_PACK_FAST_IN, msg_layers[1]
 * RG_PACK_FAST_CHAIN, upd_layer RG_PACK_FAST_UPD.  Returns RG_ERR_UNSUPPORTED for
 * other shapes / aggregations (use rg_mlp_chain + rg_segment_reduce).
 * workspace: rg_conv_layer_workspace_size() bytes, ZEROED before the first call (block
 * counters; every completed launch leaves them zero again, so no per-call memset; a
 * failed launch re-zeroes them).  One workspace per stream: two launches in flight on
 * different streams must not share it. */
size_t rg_conv_layer_workspace_size(void);
int rg_conv_layer_fused(const rg_layer* msg_layers, const rg_layer* upd_layer, int aggr,
                        const void* x, int ldx, const void* e, int lde, const int* seg_ptr,
                        const int* src, const int* dst, int n_nodes, void* x_out, int ld_out,
                        void* workspace, void* stream);
/* The same layer over edge-balanced work blocks: block b = destination nodes
 * [blk_nodes[2b], blk_nodes[2b+1]), *n_blocks_dev blocks (both from rg_conv_blocks; both
 * NULL = runs of 8 nodes, i.e. rg_conv_layer_fused).  Same results, better balance for
 * graphs with few, skewed-degree runs (dense radius frames). */
int rg_conv_layer_fused_blocks(const rg_layer* msg_layers, const rg_layer* upd_layer, int aggr,
                               const void* x, int ldx, const void* e, int lde,
                               const int* seg_ptr, const int* src, const int* dst, int n_nodes,
                               void* x_out, int ld_out, const int* blk_nodes,
                               const int* n_blocks_dev, void* workspace, void* stream);
/* Work blocks for rg_conv_layer_fused_blocks from the destination-major seg_ptr[N+1]:
 * every run of 8 nodes, split at node boundaries where its edge count would pass
 * max(128, E / 4096); written as (first node, end node) pairs in dequeue order, each of
 * the 8 XCD shares sorted by edge tiles, largest first.  blk_nodes: int32[2N] capacity;
 * n_blocks: int32[1] (device). */
size_t rg_conv_blocks_workspace_size(int n_nodes);
int rg_conv_blocks(const int* seg_ptr, int n_nodes, int* blk_nodes, int* n_blocks,
                   void* workspace, size_t workspace_bytes, void* stream);
/* A static schedule for the same layer: wave rank w of an n_waves-wave grid (n_waves a
 * multiple of 64: 8 waves per workgroup, 8 XCDs) owns the destination nodes
 * [wave_nodes[w], wave_nodes[w+1]), equal shares of degree + 4 per node (the block head and
 * update in edge units), and walks them in 8-node blocks with no work counters -- no
 * dequeue latency and no tail of whole blocks (one dense frame: BASELINE config 5).
 * wave_nodes: int32[n_waves + 1] (device), from rg_conv_wave_nodes once per graph.  Same
 * results as rg_conv_layer_fused (each destination's edges summed in CSR order by one wave). */
int rg_conv_wave_nodes(const int* seg_ptr, int n_nodes, int n_waves, int* wave_nodes,
                       void* stream);
int rg_conv_layer_fused_waves(const rg_layer* msg_layers, const rg_layer* upd_layer, int aggr,
                              const void* x, int ldx, const void* e, int lde,
                              const int* seg_ptr, const int* src, const int* dst, int n_nodes,
                              void* x_out, int ld_out, const int* wave_nodes, int n_waves,
                              void* workspace, void* stream);

/* ------------------------------------------- object-classifier finetuning */

/* gnn_detector.py:511-513: out[c] = argmax(bincount(node_labels[members of c])) (first
 * maximum) for the proposal clusters (cluster_ptr int32 [n+1], cluster_idx int32);
 * *bad_label (device int32, caller-zeroed) is set when a label is outside [0, n_classes). */
int rg_cluster_majority_label(const int64_t* node_labels, const int* cluster_ptr,
                              const int* cluster_idx, int n_clusters, int n_classes,
                              int64_t* out, int* bad_label, void* stream);
/* Loss_Object_Class (loss.py:79-89): sum_r CE(logits_r, one_hot(label_r)) / n, and
 * compute_accuracy (gnn_detector.py:24-28); loss, accuracy: device float32 [1] */
int rg_cross_entropy(const float* logits, int ld, const int64_t* labels, int n, int nc,
                     float* loss, float* accuracy, void* stream);
/* its gradient: d_logits = g (softmax - one_hot) / n, g a device float32 scalar */
int rg_cross_entropy_backward(const float* logits, int ld, const int64_t* labels, int n, int nc,
                              const float* g, float* d_logits, int ld_d, void* stream);

/* ------------------------------------------- frame-wide normalisations */

/* layer_normalization (groups = 1) / group_normalization (groups = G) of
 * modules/neural_net/common.py:223-253 over row segments (one segment = one frame's rows,
 * the tensor the reference normalises) + the block's activation:
 *   out[r][c] = [residual[r][c] +] act(std_param * (z[r][c] - mean_{s,g}) / (std_{s,g} + 1e-5)
 *               + mu_param),
 * mean / unbiased std over the segment's rows x group g's C/G features.  seg_ptr: device
 * int32 [n_seg+1]; z and out float32 [rows][C] (may alias); residual optional (the conv
 * block's identity, gnn_blocks.py:109).  Deterministic. */
size_t rg_frame_norm_workspace_size(int n_seg, int groups);
int rg_frame_norm(const float* z, int ldz, int C, int groups, const int* seg_ptr, int n_seg,
                  const float* norm_mu, const float* norm_std, int act, const float* residual,
                  int ld_res, float* out, int ld_out, void* workspace, size_t workspace_bytes,
                  void* stream);
/* Backward of rg_frame_norm (training through common.py:223-253, loss.backward()): from
 * the saved pre-norm rows z and the gradient da of the activation output, writes
 * dz = d out / d z (float32 [rows][C]) and ADDS the gradients of the scalar std / mu
 * parameters to *d_std / *d_mu (device float32[1] each, nullable together).  The segment
 * statistics are recomputed as rg_frame_norm computes them; every sum runs in float64 in
 * a fixed order (deterministic). */
size_t rg_frame_norm_backward_workspace_size(int n_seg, int groups);
int rg_frame_norm_backward(const float* z, int ldz, const float* da, int ldda, int C, int groups,
                           const int* seg_ptr, int n_seg, const float* norm_mu,
                           const float* norm_std, int act, float* dz, int lddz, float* d_mu,
                           float* d_std, void* workspace, size_t workspace_bytes, void* stream);
/* out[t] = table[idx[t]], t < n (device int32; per-frame edge offsets =
 * seg_ptr[frame_ptr]) */
int rg_gather_i32(const int* table, const int* idx, int n, int* out, void* stream);
/* out[t] = first position p in sorted[0..n) with sorted[p] >= queries[t] (n from
 * n_sorted_dev when non-NULL, capped at n_sorted): per-frame offsets of rows sorted by
 * node (link pairs by source, clusters by first member).  out int32[n_queries]; n when every
 * value is smaller. */
int rg_lower_bound_i32(const int* sorted, const int* n_sorted_dev, long n_sorted,
                       const int* queries, int n_queries, int* out, void* stream);

/* ----------------------------------------------------- segment reductions */

/* out[s][c] = reduce_{p in [seg_ptr[s], seg_ptr[s+1])} src[row(p)][c], row(p) =
 * idx ? idx[p] : p.  Sum in segment order (== the reference CPU scatter_add_ order
 * for a destination-major CSR), mean = sum / max(count,1), max with empty -> 0
 * (PyG scatter_reduce include_self=False).  src dtype RG_F32/RG_BF16, out float32
 * or bf16; C <= 256. */
int rg_segment_reduce(const void* src, int src_dtype, int ld_src, const int* seg_ptr,
                      const int* idx, int n_seg, int C, int op, void* out, int out_dtype,
                      int ld_out, void* stream);

/* Longest-first schedule for rg_segment_reduce_ordered: order int32[n_seg] = a
 * permutation of the segments by length (seg_ptr[s+1] - seg_ptr[s], capped at 255),
 * descending (a counting sort in one workgroup; ties in timing order).  Computed once
 * per graph, reused by every layer's aggregation.  workspace:
 * rg_segment_order_workspace_size() bytes (currently 0; may be NULL). */
size_t rg_segment_order_workspace_size(void);
int rg_segment_order(const int* seg_ptr, int n_seg, int* order, void* workspace,
                     size_t workspace_bytes, void* stream);
/* rg_segment_reduce (no row index, C a multiple of 64) with lane group i reducing
 * segment order[i]: the segments one wave holds then have similar lengths (a wave waits
 * for its longest).  Graphs of more than 65 536 segments keep the plain order (their
 * rows' locality is worth more: M's kNN CSR).  Same results as rg_segment_reduce, bit for bit: every segment is
 * still summed from its first row in order.  Replaces the PyG aggregation scatter at
 * edge_index[1] (gnn_blocks.py:57, 106) like rg_segment_reduce. */
int rg_segment_reduce_ordered(const void* src, int src_dtype, int ld_src, const int* seg_ptr,
                              const int* order, int n_seg, int C, int op, void* out,
                              int out_dtype, int ld_out, void* stream);
/* rg_segment_reduce / _ordered (order nullable) with an explicit schedule instead of the
 * measured defaults: groups = segments per lane group of the streaming kernel (0: the
 * one-segment-per-group kernel), rows_in_flight per lane, narrow_lanes = 1: 16-bit rows
 * as 8-B lane loads.  Compiled schedules: groups 0; (1, 4 / 8 / 12 / 16); (2, 4 / 8);
 * (4, 8); with an order, groups 1 only -- anything else returns RG_ERR_UNSUPPORTED.  Same
 * results, bit for bit, under every schedule (the parity tests sweep them; the library's
 * own entries never read the environment). */
int rg_segment_reduce_sched(const void* src, int src_dtype, int ld_src, const int* seg_ptr,
                            const int* order, int n_seg, int C, int op, void* out, int out_dtype,
                            int ld_out, int groups, int rows_in_flight, int narrow_lanes,
                            void* stream);

/* The same reductions over explicit row ranges [seg_begin[s], seg_end[s]) of src
 * [n_rows] (ranges may overlap): the per-object max-pool of the classifier GNN, whose
 * reference ranges are not a CSR (classifier/classifier.py:60-68, see
 * rg_object_row_ranges) and overlap heavily.  For op = max with a workspace of
 * rg_segment_reduce_ranges_workspace_size() bytes, a first pass writes 32-row block
 * maxima and a long range reads its head rows, its whole blocks and its tail rows
 * (exact); without one every row of every range is read. */
size_t rg_segment_reduce_ranges_workspace_size(long n_rows, int C, int src_dtype);
int rg_segment_reduce_ranges(const void* src, int src_dtype, int ld_src, long n_rows,
                             const int* seg_begin, const int* seg_end, int n_seg, int C, int op,
                             void* out, int out_dtype, int ld_out, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ------------------------------------------- cluster-level classifier GNN */

/* compute_edge_index (data_generator/datagen_classifier.py:124-133): block-diagonal
 * union of complete graphs, one per object of object_size[c] (int64) measurements,
 * no self loops, np.nonzero order.  n_nodes = sum(object_size), n_edges =
 * sum(n (n - 1)).  row_ptr int32[n_nodes+1], col int32[n_edges] (nullable),
 * edge_index int64[2][n_edges] (nullable).  The graph is symmetric: the CSR is also
 * the destination-major view rg_segment_reduce reads.  n_nodes may exceed
 * sum(object_size): the rows past the last object have no edges (row_ptr = n_edges there);
 * it must not be smaller, and n_edges must be the exact total. */
size_t rg_object_graph_workspace_size(int n_obj);
int rg_object_complete_graph(const int64_t* object_size, int n_obj, int n_nodes, long n_edges,
                             int* row_ptr, int* col, int64_t* edge_index, void* workspace,
                             size_t workspace_bytes, void* stream);

/* Pooling ranges of the classifier's Model_Inference.forward (classifier.py:60-68),
 * for a batch of samples: sample s owns objects [sample_obj_ptr[s], sample_obj_ptr[s+1])
 * and its rows start at sample_node_base[s] (both int32; NULL = one sample at row 0).
 * Per sample: begin[0] = 0, begin[c] = object_size[c-1], end = cumsum(object_size),
 * each + the sample's row base -- the reference's startidx, reproduced as written.
 * int32 [n_obj] each (nothing is written at n_obj = 0); an empty sample owns no object and
 * is skipped; workspace rg_object_graph_workspace_size(n_obj). */
int rg_object_row_ranges(const int64_t* object_size, int n_obj, const int* sample_obj_ptr,
                         const int* sample_node_base, int n_samples, int* begin, int* end,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Classifier Loss (classifier/loss.py:5-14): torchvision sigmoid_focal_loss with
 * alpha = -1, gamma = 2 on one-hot targets, summed over classes, averaged over the
 * n objects.  logits f32 [n][ld], labels int64 [n]; out f32 [1].  One workgroup,
 * fixed-order f64 reduction (deterministic). */
int rg_object_focal_loss(const float* logits, int ld, const int64_t* labels, int n, int nc,
                         float* out, void* stream);
/* Its gradient: d_logits[n][ldd] = (g_loss[0] / n) * d(loss_row)/d(logits) (g_loss: f32 [1]
 * on the device, the upstream gradient of the scalar loss). */
int rg_object_focal_loss_backward(const float* logits, int ld, const int64_t* labels, int n,
                                  int nc, const float* g_loss, float* d_logits, int ldd,
                                  void* stream);
/* Backward of the classifier's per-object channel max over rows [begin[o], end[o])
 * (classifier/blocks.py:171-176, torch.max(dim=0)): dx[first argmax row][c] +=
 * d_pooled[o][c] (atomic: the reference's ranges overlap).  x, dx f32. */
int rg_range_max_backward(const float* x, int ldx, int C, const int* begin, const int* end,
                          int n_obj, const float* d_pooled, int ldp, float* dx, int lddx,
                          void* stream);
/* The same without atomics: a row's gradients are added in object order by the one thread that
 * owns its channel -- bit-reproducible, which the atomic form is not once three objects share a
 * row.  workspace: rg_range_max_backward_ordered_workspace_size(n_obj, C) bytes (the argmax row
 * of every (object, channel)). */
size_t rg_range_max_backward_ordered_workspace_size(int n_obj, int C);
int rg_range_max_backward_ordered(const float* x, int ldx, int C, const int* begin,
                                  const int* end, int n_obj, const float* d_pooled, int ldp,
                                  float* dx, int lddx, void* workspace, size_t workspace_bytes,
                                  void* stream);
/* Backward of PyG aggr='max' (scatter_reduce amax, include_self=False) over a
 * destination-major CSR whose position p is message row p: d_msg[p][c] = d_agg[s][c] /
 * (number of maxima) for the messages equal to the segment maximum, else 0 (torch's
 * amax backward).  f32. */
int rg_segment_amax_backward(const float* msg, int ldm, int C, const int* seg_ptr, int n_seg,
                             const float* d_agg, int ldd, float* d_msg, int ldo, void* stream);


/* ------------------------------------------------------------ real-data front-end */

/* read_data.extract_and_sync_radar_data + extract_frame (read_data.py:227-303, 442-486)
 * for a window of n_scans scans already in device memory (measurements of scan s at
 * [scan_ptr[s], scan_ptr[s+1])): the stationary gate of identify_stationary_measurements
 * (meas_selection.py:22-70, 169-200, |predicted - measured range rate| <= gamma; RANSAC
 * below), vr_cartesian_vf (meas_sync.py:15-20) and the ego compensation into the
 * window's current scan (meas_sync.py:23-103), float32 outputs.  A batch of windows is
 * one call: scan_ref[s] = the current scan of scan s's window (NULL: one window whose
 * current scan is the last).  mount: f64 [n_scans][3] (x, y, yaw); odometry: f64
 * [n_scans][5] (x_seq, y_seq, yaw_seq, vx, yaw_rate).  stationary: u8 [n_meas]. */
int rg_frontend_sync(const float* x_cc, const float* y_cc, const float* azimuth_sc,
                     const float* vr, const float* vr_compensated, const int* scan_ptr,
                     int n_scans, const int* scan_ref, const double* mount,
                     const double* odometry,
                     float gamma_stationary, int n_meas, float* px, float* py, float* vx,
                     float* vy, uint8_t* stationary, void* stream);
/* RANSAC stationary-measurement rejection (meas_selection.py:96-166, applied by
 * identify_stationary_measurements to each scan's gated measurements, :188-199), in two
 * calls around the host's random draws (the reference draws np.random.shuffle consensus
 * sets; the host draws the same from numpy's generator, so a seeded generator reproduces
 * the reference):
 *   rg_frontend_gate_lists: gated_idx [n_meas] receives, at each scan's offset scan_ptr[s],
 *     the indices of the scan's measurements whose stationary flag is set, in order;
 *     gated_cnt [n_scans] their count.
 *   rg_frontend_ransac: for each scan with more than min_num_meas gated measurements,
 *     consensus_sets [n_scans][n_iter][n_samples] (positions 0 .. gated_cnt[s) - 1 in the
 *     scan's gated list) -> per set the least-squares sensor velocity (:72-93) and its
 *     inliers (|vr - predicted| <= error_margin) among the other gated measurements; the
 *     first set with the most inliers then sets the gated measurements' stationary flags
 *     (float64 arithmetic over float32 cos / sin, as numpy).  Scans with <= min_num_meas
 *     gated measurements: every flag 0 (the reference's empty inlier set).  in_ratio
 *     [n_scans] f64 = (inliers + n_samples) / gated (0 when skipped), is_valid [n_scans] u8
 *     = in_ratio >= ratio_threshold.  n_iter <= 256. */
int rg_frontend_gate_lists(const uint8_t* stationary, const int* scan_ptr, int n_scans,
                           int* gated_idx, int* gated_cnt, void* stream);
/* Host only (no device work): the consensus sets numpy's legacy generator would draw, for
 * gated_cnt [n_scans] (host) -- per scan with more than min_num_meas, n_iter in-place
 * np.random.shuffle passes over arange(count) (MT19937 + masked-rejection random_interval,
 * numpy/random/mtrand.pyx, distributions.c), the first n_samples of each -- into
 * consensus_sets [n_scans][n_iter][n_samples] (host).  mt_key [624] / *mt_pos: numpy's
 * np.random.get_state()[1] / [2], advanced in place exactly as the shuffles would (write
 * them back with np.random.set_state). */
int rg_ransac_consensus_sets(uint32_t* mt_key, int* mt_pos, const int* gated_cnt, int n_scans,
                             int n_iter, int n_samples, int min_num_meas, int* consensus_sets);
int rg_frontend_ransac(const float* azimuth_sc, const float* vr, const int* scan_ptr, int n_scans,
                       const int* gated_idx, const int* gated_cnt, const int* consensus_sets,
                       int n_iter, int n_samples, double error_margin, int min_num_meas,
                       double ratio_threshold, uint8_t* stationary, double* in_ratio,
                       uint8_t* is_valid, void* stream);
/* compute_ground_truth (compute_node_labels.py:50-105): class labels (tracked: the
 * old -> new label id map, labels.py:90-100; untracked: FALSE = 6 / STATIC = 7 by the
 * stationary flag) and offsets to each track's mean position (track_key int32, 0 = no
 * track, keys <= n_tracks).  f32 outputs. */
size_t rg_frontend_labels_workspace_size(int n_tracks);
int rg_frontend_labels(const int* track_key, int n_tracks, const int64_t* label_id,
                       const uint8_t* stationary, const int* old_to_new, int n_old,
                       const float* px, const float* py, int n_meas, float* cls,
                       float* offset_x, float* offset_y, void* workspace,
                       size_t workspace_bytes, void* stream);
/* select_meas_within_the_grid (grid_features.py:162-174) + select_moving_data
 * (graph_features.py:167-182): index[0..*n_selected) = the measurements inside
 * [min_x, max_x) x [min_y, max_y) whose class is not static_id, in order.  With a batch
 * of windows (measurements of window w at [win_ptr[w], win_ptr[w+1])), frame_ptr
 * [n_windows + 1] receives each window's range of selected rows (the graph build's
 * frame_ptr); both may be NULL. */
size_t rg_frontend_select_workspace_size(int n_meas);
int rg_frontend_select(const float* px, const float* py, const float* cls, int n_meas,
                       float min_x, float max_x, float min_y, float max_y, float static_id,
                       const int* win_ptr, int n_windows, int* frame_ptr, int* index,
                       int* n_selected, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------ sequence store */

/* A RadarScenes sequence resident in device memory (sequence.py, SequenceStore): what
 * read_data.get_sequence_data (read_data.py:416-439) returns, uploaded once.  scenes: int32
 * [n_scenes][4] in chain order = (begin, end) of the scene's rows in the measurement arrays
 * (radar_indices; may be empty, need not be contiguous or ascending), its row of the mount
 * table and its row of the odometry table.  mount: f64 [n_sensors][3] (x, y, yaw); odometry:
 * f64 [n_odometry][5] (x_seq, y_seq, yaw_seq, vx, yaw_rate).  Measurement arrays of n_meas
 * rows: six f32 fields, timestamp int64, sensor_id / label_id u8 (as the .h5 files hold them),
 * track_key int32 (0 = the empty track id, else 1..n_tracks). */
typedef struct rg_sequence {
  const int* scenes;
  const double* mount;
  const double* odometry;
  const float* x_cc;
  const float* y_cc;
  const float* azimuth_sc;
  const float* vr;
  const float* vr_compensated;
  const float* rcs;
  const int64_t* timestamp;
  const uint8_t* sensor_id;
  const uint8_t* label_id;
  const int* track_key;
  int n_scenes, n_sensors, n_odometry, n_meas, n_tracks;
} rg_sequence;

/* The windows cut from a sequence, the batch layout of rg_frontend_sync: n_windows * W
 * window-scans j = b * W + w.  scan_ptr int32 [n_windows * W + 1], scan_ref int32
 * [n_windows * W] (the window's last scan), win_ptr int32 [n_windows + 1], mount f64
 * [n_windows * W][3], odometry f64 [n_windows * W][5]; per output measurement (capacity rows
 * each) meas_scan int32 (its window-scan), src_row int32 (its row in the sequence), the six
 * f32 fields, timestamp, sensor_id and label_id int64, track_key int32. */
typedef struct rg_window_batch {
  int* scan_ptr;
  int* scan_ref;
  int* win_ptr;
  double* mount;
  double* odometry;
  int* meas_scan;
  int* src_row;
  float* x_cc;
  float* y_cc;
  float* azimuth_sc;
  float* vr;
  float* vr_compensated;
  float* rcs;
  int64_t* timestamp;
  int64_t* sensor_id;
  int64_t* label_id;
  int* track_key;
} rg_window_batch;

/* create_dataset_sliding_window + the slicing of extract_and_sync_radar_data
 * (read_data.py:203-224, 250-291) for a batch of windows, on the device: window b holds the
 * W scenes win_first[b] .. win_first[b] + W - 1 (win_first: int32 [n_windows], device;
 * repeats and overlaps allowed).  Two launches, no host synchronisation: a one-workgroup
 * scan of the n_windows * W scene sizes writes the per-window-scan outputs, then one wave per
 * window-scan copies its rows: output row m of window-scan j comes from sequence row
 * scenes[s][0] + (m - scan_ptr[j]); its key is k == 0 ? 0 : k + b * n_tracks (the same track
 * in two windows of a batch stays two tracks).  capacity = the rows the per-measurement
 * outputs hold (the host's sum of the scene sizes): rows at or beyond it, or beyond the
 * computed scan_ptr[n_windows * W], are never written, and a scene range is cut to
 * [0, n_meas) before it is read; a window-scan whose scene, sensor row or odometry row lies
 * outside its table is empty with a NaN pose.  RG_ERR_ARG, launching nothing: a NULL
 * pointer, a negative size, W < 1, n_windows * W or n_windows * n_tracks beyond int32. */
int rg_sequence_windows(const rg_sequence* seq, const int* win_first, int n_windows, int W,
                        long capacity, const rg_window_batch* out, void* stream);

/* The windows of a batch cut from several sequences (sequence.py, SequenceSet): window b is
 * W consecutive scenes of sequence win[2b] starting at scene win[2b+1].  seqs is a DEVICE
 * array of n_seq rg_sequence descriptors (8-byte aligned), win a device int32 [n_windows][2].
 * The outputs, the two launches and every clamp are rg_sequence_windows': each descriptor's
 * tables are read as that entry point reads its one sequence's, src_row is the row inside
 * the window's own sequence, and the non-zero track keys of window b become
 * k + b * key_stride (key_stride >= the largest n_tracks keeps the windows' keys apart).  A
 * sequence id outside [0, n_seq) makes the window's scans empty with NaN poses; nothing is
 * read for it.  The descriptors' own sizes and pointers lie on the device and are not
 * validated on the host: a size <= 0 makes that table empty.  RG_ERR_ARG, launching
 * nothing: a NULL pointer, n_seq < 1, key_stride < 0, W < 1, a negative n_windows or
 * capacity, n_windows * W or n_windows * key_stride beyond int32. */
int rg_sequence_set_windows(const rg_sequence* seqs, int n_seq, int key_stride, const int* win,
                            int n_windows, int W, long capacity, const rg_window_batch* out,
                            void* stream);

/* ------------------------------------------------------------ training feed */

/* The x-axis flip augmentation of get_data_for_datagen (read_data.py:522-524) for a batch of
 * windows: py and vy (f32 [n_meas], rg_frontend_sync's outputs) are negated in place over
 * [win_ptr[w], win_ptr[w + 1]) for every window w with flip[w] != 0 (flip: u8 [n_windows],
 * device); the other windows' values are not written.  win_ptr == NULL: one window covering
 * [0, n_meas).  It runs between rg_frontend_sync and rg_frontend_labels / rg_frontend_select,
 * where the reference flips, so the offsets and the grid test see the flipped values.  One
 * launch, no host synchronisation; n_meas == 0 or n_windows == 0 launches nothing.
 * RG_ERR_ARG, launching nothing: a negative size, a NULL pointer with n_meas > 0, or
 * win_ptr == NULL with n_windows > 1. */
int rg_frontend_flip(float* py, float* vy, const int* win_ptr, int n_windows,
                     const uint8_t* flip, int n_meas, void* stream);

/* The label tensors of RadarScenesDataset.__getitem__ (datagen_gnn.py:126-134) for a batch of
 * dynamic frames, one launch: node_class int64 [n_nodes] from the f32 class_labels,
 * node_offsets f32 [n_nodes][2] = (offset_x, offset_y) interleaved (8-byte aligned) and
 * edge_class int64 [pair_capacity], the labels of compute_edge_labels.compute_ground_truth
 * (compute_edge_labels.py:7-20) in link-pair order: for p < *n_pairs (the device count
 * rg_link_pairs wrote, cut to pair_capacity) 1 when track_key[pair_src[p]] ==
 * track_key[pair_dst[p]] and that key is not 0 (no track), else 0; 0 for every p in
 * [*n_pairs, pair_capacity) and for a pair with an endpoint outside [0, n_nodes).  (The
 * reference reads the labels at nonzero(triu(adj, 1)) out of a matrix filled over adj_list =
 * where(adj): every such pair is an edge with src < dst, so no matrix is needed.)  No host
 * synchronisation; n_nodes == 0 and pair_capacity == 0 launch nothing.  RG_ERR_ARG, launching
 * nothing: a negative size, n_nodes * 2 or pair_capacity beyond int32, a NULL node array with
 * n_nodes > 0, a NULL pair array with pair_capacity > 0. */
int rg_train_labels(const float* class_labels, const float* offset_x, const float* offset_y,
                    int n_nodes, const int* track_key, const int* pair_src, const int* pair_dst,
                    const int* n_pairs, long pair_capacity, int64_t* node_class,
                    float* node_offsets, int64_t* edge_class, void* stream);

/* generate_gt_offset (compute_node_labels.py:50-67) with the mean numpy takes: offset_x[i] =
 * mean(px of i's track) - px[i] (offset_y alike; 0 where track_key[i] is 0 or outside
 * [1, n_tracks]), the mean being np.mean of the track's float32 values in measurement order
 * -- a float32 pairwise sum (numpy's blocks of 128, eight interleaved partial sums) over the
 * count -- so the offsets equal the reference's bit for bit.  rg_frontend_labels takes the
 * mean in float64, within an ulp of this one; a training label is compared exactly, so the
 * training feed overwrites rg_frontend_labels' offsets with these.  It runs after
 * rg_frontend_flip.  Three launches (first index and count per key, one wave per key for the
 * mean, the offsets); no host synchronisation; n_meas == 0 launches nothing.  RG_ERR_ARG,
 * launching nothing: a negative size, a NULL array with n_meas > 0, a workspace smaller than
 * rg_train_offsets_workspace_size(n_tracks) or not 8-byte aligned. */
size_t rg_train_offsets_workspace_size(int n_tracks);
int rg_train_offsets(const int* track_key, int n_tracks, const float* px, const float* py,
                     int n_meas, float* offset_x, float* offset_y, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------ proposal branch */

/* Predicted cluster centres (gnn_detector.py:164-167): unnormalize_gt_offsets
 * (compute_offsets.py:13-17, offset * sigma + mu) added to other_features[:, :2];
 * float32, no FMA.  offsets: f32 [N][ld_off] (node_offsets_predictions), xy: f32
 * [N][ld_xy]; cx, cy: f32 [N]. */
int rg_proposal_centres(const float* offsets, int ld_off, const float* xy, int ld_xy, int n_nodes,
                        float mu_x, float mu_y, float sigma_x, float sigma_y, float* cx,
                        float* cy, void* stream);

/* Connected components of the eps-graph on the centres, per frame
 * (Simple_DBSCAN with compute_adjacency_mat_from_predicted_offsets, clustering.py:26-93:
 * an edge where the SQUARED distance <= eps2).  labels: int32 [N], label = the
 * component's lowest global node index. */
size_t rg_cluster_radius_workspace_size(int n_nodes, int n_frames, int max_frame_nodes);
int rg_cluster_radius(const float* px, const float* py, const int* frame_ptr, int n_nodes,
                      int n_frames, int max_frame_nodes, float eps2, int* labels,
                      void* workspace, size_t workspace_bytes, void* stream);

/* Connected components over predicted links (compute_adjacency_mat_from_predicted_edges,
 * clustering.py:8-23): pair p = (pair_src[p], pair_dst[p]) is an edge when
 * link_logits[p][1] > link_logits[p][0] (the argmax of gnn_detector.py:158-159) and
 * sqrt(dx^2 + dy^2) < eps on the centres.  labels as rg_cluster_radius. */
int rg_cluster_pairs(const float* px, const float* py, const int* pair_src, const int* pair_dst,
                     const int* n_pairs_dev, long n_pairs, const float* link_logits,
                     int ld_logits, float eps, int n_nodes, int* labels, void* stream);

/* Cluster ids in the reference's order (ascending lowest node index; frames are
 * concatenated, each numbered from its own first cluster) and the member lists,
 * ascending (gnn_detector.py:180-184): cluster_of int32 [N], cluster_ptr int32 [N+1]
 * (entries past *n_clusters repeat N; exactly N + 1 entries are written), cluster_idx
 * int32 [N], *n_clusters device int.  labels[i] <= i is the lowest node of i's component,
 * as rg_cluster_radius / rg_cluster_pairs write it. */
size_t rg_cluster_lists_workspace_size(int n_nodes);
int rg_cluster_lists(const int* labels, int n_nodes, int* cluster_of, int* cluster_ptr,
                     int* cluster_idx, int* n_clusters, void* workspace, size_t workspace_bytes,
                     void* stream);

/* ---------------------------------------------------------------- evaluation */
/* Detection and segmentation evaluation (modules/performance/detection_accuracy.py,
 * performance_eval_detection.ipynb, performance_eval_segmentation.ipynb) for a batch of
 * frames: global node ids and frame_ptr int32 [n_frames + 1] as rg_cluster_radius, every
 * launch on the given stream, no host synchronisation.  Cluster CSRs have the form of
 * rg_cluster_lists: cluster_ptr int32 [N + 1] whose entries past the last cluster repeat N,
 * clusters ordered by frame. */

/* compute_node_idx_for_each_cluster (datagen_gnn.py:15-45) from track_key int32 [N] (0 = no
 * track; keys rank the sorted unique track ids, so ascending keys are np.unique's order):
 * per frame the tracked clusters in ascending key order, then one singleton per untracked
 * node in node order; members ascending; cluster_class int64 [N] = node_class of the lowest
 * member.  frame_clusters int32 [n_frames] = clusters per frame, *n_clusters device int. */
size_t rg_eval_gt_clusters_workspace_size(int n_nodes);
int rg_eval_gt_clusters(const int* track_key, const int64_t* node_class, const int* frame_ptr,
                        int n_nodes, int n_frames, int* cluster_of, int* cluster_ptr,
                        int* cluster_idx, int* frame_clusters, int64_t* cluster_class,
                        int* n_clusters, void* workspace, size_t workspace_bytes, void* stream);

/* out[r] = index of the first maximum of row r of x (float32 [n_rows][ld]); the predicted
 * class of detection_accuracy.py:97-98 / 108-109 without the softmax. */
int rg_argmax_rows(const float* x, int ld, long n_rows, int n_cols, int64_t* out, void* stream);

/* cluster_of int32 [n_nodes] of a cluster CSR (cluster_ptr int32 [n_clusters + 1]): the
 * cluster of every member, -1 for a node in none. */
int rg_eval_cluster_of(const int* cluster_ptr, const int* cluster_idx, int n_clusters,
                       int n_nodes, int* cluster_of, void* stream);

/* compute_gt_and_pred_associations (detection_accuracy.py:192-273, 'inv_iou') after the size
 * filter of detection_accuracy.py:141-164 (a cluster is kept when size > size_threshold),
 * for every frame at once.  *_of int32 [N] (-1 = in no cluster), *_ptr int32 [N + 1], *_idx
 * int32 [N].  Outputs: gt_kept / pred_kept int32 [N] flags per cluster; per frame f its picks
 * in pick order at slots [pick_start[f], pick_start[f] + pick_count[f]) of the [N] arrays:
 * pick_gt / pick_pred = indices among the frame's kept clusters, pick_d = float32(1 - IoU),
 * pick_positive = d <= eps, pick_gt_cluster / pick_pred_cluster = the cluster ids in the CSRs
 * (-1 in every unused slot).  A frame without a kept cluster on either side has no picks.
 * max_frame_nodes >= 2^24 returns RG_ERR_UNSUPPORTED (1 - 1/union would round to 1.0f). */
size_t rg_eval_associate_workspace_size(int n_nodes, int n_frames);
int rg_eval_associate(const int* frame_ptr, int n_nodes, int n_frames, int max_frame_nodes,
                      const int* gt_of, const int* gt_ptr, const int* gt_idx, const int* pred_of,
                      const int* pred_ptr, const int* pred_idx, int size_threshold, float eps,
                      int* gt_kept, int* pred_kept, int* pick_start, int* pick_count,
                      int* pick_gt, int* pick_pred, float* pick_d, int* pick_positive,
                      int* pick_gt_cluster, int* pick_pred_cluster, void* workspace,
                      size_t workspace_bytes, void* stream);

/* The same association under the 'l2_norm' criterion (detection_accuracy.py:211-213, 225): the
 * G x P matrix of a frame's kept clusters holds the Euclidean distance between their centres,
 * gt_mu / pred_mu float32 [N][2] indexed by cluster id (the mu of rg_cluster_stats over the
 * padded CSRs; an empty slot is never read).  min(G, P) rounds: a round picks the minimum of
 * the remaining matrix, on equal distances the lowest row and then the lowest column
 * (np.nonzero(dist == np.min(dist))[0]), and the picked row and column leave the matrix.
 * Arithmetic: d = sqrt(fl(fl(dx dx) + fl(dy dy))) in float32, two rounded products, one add, a
 * correctly rounded square root, never contracted: numpy's np.linalg.norm(.., axis=-1) bit for
 * bit.  pick_d = d, pick_positive = d <= eps; every output has the layout of
 * rg_eval_associate, so rg_eval_accumulate consumes it unchanged.
 * Domain: a frame with picks to make in which a kept cluster's centre is not finite gets no
 * picks and sets *bad_value (device int32, caller-zeroed; the reference raises there).
 * Distances of 9,999,999 or more meet the reference's VERY_LARGE_NUM sentinel and are outside
 * the domain (picks stay well defined here).
 * Cost: the matrix is never stored (workspace O(N + F)).  One workgroup per frame recomputes
 * distances from the centres: G P up front, P per row whose cached nearest column was taken
 * by another row -- O(min(G, P) G P) in the worst case, where every row keeps wanting the same
 * column.  max_frame_nodes (an upper bound of a frame's clusters a side) sizes the LDS of the
 * launch; a frame with more than 4096 kept clusters a side, or more than max_frame_nodes,
 * keeps its state in the workspace instead. */
size_t rg_eval_associate_l2_workspace_size(int n_nodes, int n_frames);
int rg_eval_associate_l2(const int* frame_ptr, int n_nodes, int n_frames, int max_frame_nodes,
                         const int* gt_ptr, const int* gt_idx, const int* pred_ptr,
                         const int* pred_idx, int size_threshold, float eps, const float* gt_mu,
                         const float* pred_mu, int* gt_kept, int* pred_kept, int* pick_start,
                         int* pick_count, int* pick_gt, int* pick_pred, float* pick_d,
                         int* pick_positive, int* pick_gt_cluster, int* pick_pred_cluster,
                         int* bad_value, void* workspace, size_t workspace_bytes, void* stream);

/* performance_eval_detection.ipynb: confusion[gt][pred] += 1 per pick (a negative pick's gt
 * class is false_class), gt_count[class] += 1 per kept ground-truth cluster, pred_count[class]
 * += 1 per kept predicted cluster; int64 device accumulators ([nc][nc], [nc], [nc]) kept by
 * the caller across batches.  *bad_class (device int32, caller-zeroed) is set when a class
 * is outside [0, num_classes).  num_classes outside 1..32: RG_ERR_UNSUPPORTED. */
int rg_eval_accumulate(const int* pick_gt_cluster, const int* pick_pred_cluster,
                       const int* pick_positive, const int* gt_kept, const int* pred_kept,
                       const int64_t* gt_class, const int64_t* pred_class, int n_nodes,
                       int num_classes, int false_class, int64_t* confusion, int64_t* gt_count,
                       int64_t* pred_count, int* bad_class, void* stream);

/* performance_eval_segmentation.ipynb: confusion[node_class][argmax(node_logits)] += 1 and
 * gt_count[node_class] += 1 over all nodes; accumulators and bad_class as above. */
int rg_eval_node_confusion(const float* node_logits, int ld, const int64_t* node_class,
                           long n_nodes, int num_classes, int64_t* confusion, int64_t* gt_count,
                           int* bad_class, void* stream);

/* rg_eval_node_confusion for predictions that are class ids already (a cluster's majority
 * class, the classes of rg_cluster_class_from_objects): confusion[gt_class[r]][pred_class[r]]
 * += 1 and gt_count[gt_class[r]] += 1 over the n rows; accumulators as above.  A row with
 * either class outside [0, num_classes) sets *bad_class (device int32, caller-zeroed) and is
 * skipped.  num_classes outside 1..32: RG_ERR_UNSUPPORTED; n < 0: RG_ERR_ARG. */
int rg_eval_class_confusion(const int64_t* gt_class, const int64_t* pred_class, long n,
                            int num_classes, int64_t* confusion, int64_t* gt_count,
                            int* bad_class, void* stream);

/* ------------------------------------------------------------------ object stage */
/* From the detector's clusters to the classifier's inputs and the object list
 * (modules/inference/inference.py, ellipse.py, output.py:99-171,
 * data_generator/datagen_classifier.py:35-124, 166-190) for a batch of frames: global node
 * ids, frame_ptr int32 [n_frames + 1], cluster CSRs of the rg_cluster_lists form (clusters
 * ordered by frame, none empty).  Every launch on the given stream, no host synchronisation;
 * matrices are row-major float32. */

/* compute_cluster_sample_mean_and_cov (inference.py:23-30) of every cluster from xy f32
 * [N][ld_xy]: size int32 [K], mu [K][2] = (sum p) / n, sigma [K][2][2] = sum (mu - p)(mu - p)^T
 * / (n - 1) + noise_cov (n == 1: noise_cov).  noise_cov: HOST float32 [4], symmetric.  Sums run
 * over the members in list order in float32 without contraction: bit-identical to numpy.
 * eigval [K][2] / eigvec [K][2][2] (columns; both nullable): np.linalg.eig of sigma in float32,
 * in LAPACK's order and sign (slanv2).  *bad_index (device int32, caller-zeroed, nullable) is
 * set when a member or an offset lies outside [0, n_nodes]. */
int rg_cluster_stats(const float* xy, int ld_xy, int n_nodes, const int* cluster_ptr,
                     const int* cluster_idx, int n_clusters, const float* noise_cov, int* size,
                     float* mu, float* sigma, float* eigval, float* eigvec, int* bad_index,
                     void* stream);

/* compute_cov_ellipse (ellipse.py:4-37) as written: abt [K][3] = half-axes a = chi_sq
 * sqrt(largest eigenvalue), b = chi_sq sqrt(smallest), theta = atan2(v[l][1], v[l][0]) of ROW
 * l = index of the largest eigenvalue (pi / 2 when v[l][0] == 0); points [K][n_points][2]
 * (nullable; needs mu) = [a cos th, b sin th] @ R^T + mu over th = linspace(0, 2 pi,
 * n_points).  n_points < 1: RG_ERR_ARG. */
int rg_cov_ellipse(const float* eigval, const float* eigvec, const float* mu, int n_clusters,
                   float chi_sq, int n_points, float* abt, float* points, void* stream);

/* torch.max(F.softmax(x, -1), -1) of output.py:104-121 per row of x f32 [n_rows][ld]: cls int64
 * = first maximum of the logits (as rg_argmax_rows), score f32 = its float32 softmax value
 * (either nullable).  num_classes outside 1..32: RG_ERR_UNSUPPORTED. */
int rg_softmax_max(const float* x, int ld, long n_rows, int num_classes, int64_t* cls,
                   float* score, void* stream);

/* The cluster-level classifier as a class source per cluster (the object class of
 * output.py:111-128, detection_accuracy.py:95-109, from the second stage): logits f32
 * [n_objects][ld] per kept object, obj_cluster int32 [n_objects] the source cluster of every
 * object (rg_object_select's).  cluster_class[obj_cluster[o]] / cluster_score[obj_cluster[o]]
 * (nullable) = what rg_softmax_max returns for row o, bit for bit (one device function); a
 * cluster that no object names gets fill_class and 0.0f.  A fill launch, then a scatter launch
 * in stream order.  The entries of obj_cluster are distinct; duplicates are outside the
 * domain (the last writer is not defined).  An entry outside [0, n_clusters) sets *bad_index
 * (device int32, caller-zeroed) and writes nothing for that object.  n_objects == 0 still
 * fills; n_clusters == 0 launches nothing.  num_classes outside 1..32: RG_ERR_UNSUPPORTED;
 * ld < num_classes or a negative count: RG_ERR_ARG. */
int rg_cluster_class_from_objects(const float* logits, int ld, long n_objects, int num_classes,
                                  const int* obj_cluster, int n_clusters, int64_t fill_class,
                                  int64_t* cluster_class, float* cluster_score, int* bad_index,
                                  void* stream);

/* remove_low_quality_proposals (datagen_classifier.py:166-190: kept when size >= min_meas) and
 * the class filter of output.py:123-128 (cluster_class[c] == drop_class is dropped; -1 = no
 * class filter), compacted on the device.  cluster_row int32 [K] = first member row of a kept
 * cluster, -1 otherwise; obj_cluster int32 [K] = source cluster of kept object o; obj_row_ptr
 * int32 [K + 1] = member rows of object o at [obj_row_ptr[o], obj_row_ptr[o + 1]);
 * frame_obj_ptr / frame_row_ptr int32 [n_frames + 1] (nullable together) = each frame's range
 * of kept objects / member rows; counts: device int64 [3] = kept objects K', member rows M',
 * edges E' = sum n (n - 1) of the per-object complete graphs. */
size_t rg_object_select_workspace_size(int n_clusters);
int rg_object_select(const int* cluster_ptr, const int* cluster_idx, int n_clusters,
                     const int* frame_ptr, int n_frames, const int64_t* cluster_class,
                     int num_classes, int min_meas, int drop_class, int* cluster_row,
                     int* obj_cluster, int* obj_row_ptr, int* frame_obj_ptr, int* frame_row_ptr,
                     int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* Rows of the kept objects o < counts[0] from the per-cluster arrays, c = obj_cluster[o]:
 * obj_size int64 (object_num_meas), obj_class int64, obj_score, obj_mu [.][2], obj_sigma
 * [.][2][2], obj_ellipse [.][3], obj_frame int32 (the frame of the first member).  Every
 * output is nullable; its source must be given. */
int rg_object_gather(const int* obj_cluster, const int64_t* counts, int n_clusters,
                     const int* size, const int64_t* cluster_class, const float* score,
                     const float* mu, const float* sigma, const float* ellipse,
                     const int* cluster_ptr, const int* cluster_idx, const int* frame_ptr,
                     int n_frames, int64_t* obj_size, int64_t* obj_class, float* obj_score,
                     float* obj_mu, float* obj_sigma, float* obj_ellipse, int* obj_frame,
                     void* stream);

/* extract_and_compute_features_and_labels (datagen_classifier.py:62-100): features f32 [M'][5],
 * one row per member of a kept cluster at cluster_row[c] + its position in the list:
 * (x, y) = (p - mu) @ eigvec, r = sqrt(x^2 + y^2), th = atan2(y, x), rcs[node * ld_rcs]. */
int rg_object_features(const float* xy, int ld_xy, const float* rcs, int ld_rcs, int n_nodes,
                       const int* cluster_ptr, const int* cluster_idx, int n_clusters,
                       const int* cluster_row, const float* mu, const float* eigvec,
                       float* features, void* stream);


/* ------------------------------------------------------------------ training */
/* The backward of the hot path (Model_Training + Loss_Graph + loss.backward(),
 * gnn_detector.py:428-478, loss.py:37-76, training.py:66-85), float32.  Forward
 * tapes come from rg_mlp_chain with rg_layer.save_pre / save_out set. */

/* Backward of channel_normalization + activation (common.py:208-220, 256-267) for
 * `rows` rows of width C: from the saved pre-normalisation z and the gradient of the
 * activation output da, dz (may alias da) and the gradients of the scalar parameters,
 * ACCUMULATED into *d_mu / *d_std (device; deterministic order).  has_norm = 0: only
 * the activation.  workspace: rg_ffn_backward_workspace_size() bytes. */
size_t rg_ffn_backward_workspace_size(void);
int rg_ffn_backward(const float* z, int ldz, const float* da, int ldda, long rows, int C,
                    int has_norm, const float* mu, const float* std_, int act, float* dz,
                    int lddz, float* d_mu, float* d_std, void* workspace, void* stream);
/* The same with the activation gradient gathered: row r reads da[gidx[r]] (times
 * gscale[gidx[r]] when gscale is non-NULL) -- d msg = d agg[dst] of the message MLP's last
 * layer (sum / mean aggregation, gnn_blocks.py:104-113) without materialising d msg;
 * the same values as rg_gather_segment_sum followed by rg_ffn_backward.  dz may not alias da. */
int rg_ffn_backward_gather(const float* z, int ldz, const float* da, int ldda, const int* gidx,
                           const float* gscale, long rows, int C, int has_norm, const float* mu,
                           const float* std_, int act, float* dz, int lddz, float* d_mu,
                           float* d_std, void* workspace, void* stream);

/* dA = dz_next W (layer: ONE transposed RG_F32 | RG_PACK_F32_FAST image, in_dim = the width of
 * dz_next, out_dim = C, as the backward's dX launches use) with the previous ffn_block's
 * channel_normalization + activation backward (common.py:208-220, 256-267) applied in the
 * same registers: dz = rg_ffn_backward(z, dA), d_mu / d_std ACCUMULATED -- dA never reaches
 * memory.  has_norm is implied (mu / std required); act RG_ACT_NONE or RG_ACT_LEAKY; (in_dim,
 * C) in {(64, 128), (128, 128), (64, 64)}, else RG_ERR_UNSUPPORTED (the caller runs the two
 * steps).  Row sums in float32, their sums over rows in float64 in a fixed order:
 * bit-reproducible.  workspace: rg_dx_norm_backward_workspace_size(rows) bytes. */
size_t rg_dx_norm_backward_workspace_size(long rows);
int rg_dx_norm_backward(const rg_layer* layer, long rows, const float* dz_next, int ld_dzn,
                        const float* z, int ldz, const float* mu, const float* std_, int act,
                        float* dz, int lddz, float* d_mu, float* d_std, void* workspace,
                        size_t workspace_bytes, void* stream);

/* Weight / bias gradient of nn.Linear (common.py:195): dW[out][in] += sum_r dz[r]^T x[r],
 * db[out] += sum_r dz[r] (db may be NULL), x[r] formed from in0/in1/in2 by in_mode as in
 * rg_mlp_chain (float32 inputs).  Rows are reduced in fixed chunks, the chunk partials
 * in a fixed order: bit-reproducible.  workspace: rg_linear_grad_workspace_size(). */
size_t rg_linear_grad_workspace_size(long rows, int out_dim, int in_dim);
int rg_linear_grad(const float* dz, int lddz, long rows, int out_dim, int in_dim, int in_mode,
                   const float* in0, int ld0, int w0, const float* in1, int ld1, int w1,
                   const float* in2, int ld2, int w2, const int* idx0, const int* idx1,
                   float* dW, float* db, void* workspace, size_t workspace_bytes, void* stream);
/* The same into a column block of a wider dW: rows ld_dw floats apart (>= in_dim). */
int rg_linear_grad_ld(const float* dz, int lddz, long rows, int out_dim, int in_dim, int in_mode,
                      const float* in0, int ld0, int w0, const float* in1, int ld1, int w1,
                      const float* in2, int ld2, int w2, const int* idx0, const int* idx1,
                      float* dW, int ld_dw, float* db, void* workspace, size_t workspace_bytes,
                      void* stream);

/* Incidence lists: for node n, every u < n_items with a[u] == n or b[u] == n (b may be
 * NULL), ascending: ptr int32 [n_nodes+1], list int32 [n_items * (b ? 2 : 1)].  An item
 * with a[u] == b[u] is listed twice, so every list entry is one (item, side) of the index
 * arrays.  At n_nodes = 0 (then n_items = 0) ptr[0] = 0 is still written.  The
 * transpose of an index_select (PyG x_j = x[edge_index[0]], the link pairs' x[i] + x[j]),
 * used to sum its gradient per node in a fixed order. */
size_t rg_incidence_workspace_size(int n_nodes, long n_items);
int rg_incidence(const int* a, const int* b, long n_items, int n_nodes, int* ptr, int* list,
                 void* workspace, size_t workspace_bytes, void* stream);

/* out[n][0:width] (+)= sum_{k in [ptr[n], ptr[n+1])} src[row(k)][col0 : col0 + width],
 * row(k) = list ? list[k] : k; scale (per row of src, may be NULL) multiplies each term
 * (PyG mean: 1 / count).  accumulate = 0 overwrites.  float32, width <= 256. */
int rg_gather_segment_sum(const float* src, int ld_src, int col0, int width, const int* ptr,
                          const int* list, const float* scale, int n_nodes, float* out,
                          int ld_out, int accumulate, void* stream);

/* Backward of the per-cluster channel max (object_classification gnn_blocks.py:384-387,
 * torch.max(dim=0)): dh[argmax_c(f)][f] += dpooled[c][f], argmax = first maximum in
 * list order.  h float32 [N][ld_h]; cluster lists as rg_segment_reduce's idx CSR. */
int rg_segment_max_backward(const float* h, int ld_h, int C, const int* cluster_ptr,
                            const int* cluster_idx, int n_clusters, const float* dpooled,
                            int ld_p, float* dh, int ld_dh, void* stream);

/* Loss_Graph.forward (loss.py:37-76) + compute_accuracy (gnn_detector.py:24-28).
 * node_cls f32 [N][nc], node_reg f32 [N][2], link f32 [U][2], obj f32 [Ncl][nc];
 * labels int64 (node_class [N], edge_class [U], obj_class [Ncl]); node_offsets f32
 * [N][2] raw (normalised inside: (o - mu) / sigma, compute_offsets.py:6-11);
 * class_w f32 [nc].  losses f32 [4] = weighted (node_cls, node_reg, edge_cls, obj_cls)
 * as loss.py:71-75, acc f32 [3] = (segment, edge, object) accuracy (device). */
typedef struct rg_loss_args {
  const float* node_cls; const float* node_reg; const float* link; const float* obj;
  const long long* node_class; const float* node_offsets; const long long* edge_class;
  const long long* obj_class; const float* class_w;
  long n_nodes; long n_pairs; long n_clusters; int n_classes;
  float mu_x, mu_y, sigma_x, sigma_y;
  float w_node_cls, w_node_reg, w_edge_cls, w_obj_cls;
} rg_loss_args;
size_t rg_loss_workspace_size(long n_nodes, long n_pairs, long n_clusters);
int rg_loss_graph(const rg_loss_args* args, float* losses, float* acc, void* workspace,
                  size_t workspace_bytes, void* stream);
/* d(sum_i g[i] * losses[i]) / d(logits) (g: device f32 [4], the upstream gradients of
 * the four losses): d_node_cls [N][nc], d_node_reg [N][2], d_link [U][2], d_obj [Ncl][nc]. */
int rg_loss_graph_backward(const rg_loss_args* args, const float* g, float* d_node_cls,
                           float* d_node_reg, float* d_link, float* d_obj, void* stream);

/* torch.optim.SGD step (dampening 0, no nesterov; set_param_for_training_gnn.py:46) on
 * flat float32 arrays: d = grad_scale g + wd p; buf = first ? d : momentum buf + d;
 * p -= lr buf.  grad_scale = 1 / world_size averages an all-reduced (summed) gradient
 * as DistributedDataParallel does; 1 on one GPU (exact). */
int rg_sgd_step(float* param, const float* grad, float* momentum_buf, long n, float lr,
                float momentum, float weight_decay, int first_step, float grad_scale,
                void* stream);

/* The optimizer step of the reference's train_model loop (training.py:66-85) with its two
 * host-side rules evaluated on the device, so a data-parallel step needs no host sync:
 *  - skip_batch (training.py:40-45, 79-85): when losses[0] + ... + losses[n_losses-1]
 *    (float32, left to right) is NaN, param and the optimizer state are left untouched and
 *    the step is not counted.  The DDP trainer all-reduces the losses in the same bucket as
 *    the gradients, so a NaN on any rank reaches every rank and all ranks skip together.
 *    losses = NULL: never skip.
 *  - MultiStepLR (set_param_for_training_gnn.py:51-56, stepped only after an applied step,
 *    training.py:83-84): applied step k (0-based) uses lr[j], j = the number of distinct
 *    milestones ms[i] <= k.  The host fills lr[] exactly as the scheduler chains it (in
 *    double: lr[j] = lr[j-1] * gamma ** multiplicity(ms[j-1])); milestones < 0 never fire
 *    and are dropped by the host, milestone 0 fires before the first step.
 * step_state: device int[2], the applied-step counter ping-ponged between launches: the
 * launch reads step_state[parity] and writes step_state[parity ^ 1]; the caller flips
 * parity every launch (both zero before the first).  The first applied step (k = 0)
 * initialises the momentum buffer (torch's momentum_buffer = None). */
#define RG_LR_MILESTONES_MAX 16
typedef struct rg_lr_schedule {
  int n_milestones;                        /* distinct, ascending, >= 0 */
  int milestones[RG_LR_MILESTONES_MAX];
  double lr[RG_LR_MILESTONES_MAX + 1];
} rg_lr_schedule;
int rg_sgd_step_sched(float* param, const float* grad, float* momentum_buf, long n,
                      const rg_lr_schedule* sched, float momentum, float weight_decay,
                      float grad_scale, const float* losses, int n_losses, int* step_state,
                      int parity, void* stream);
/* torch.optim.AdamW (set_param_for_training_gnn.py:47; amsgrad off, the foreach update
 * order) with the same skip / schedule / step_state rules (the hyper-parameters are
 * doubles, as Python holds them; each scalar is formed in double, then rounded): t = k + 1;
 * p *= 1 - lr wd; m = lerp(m, g, 1 - beta1); v = beta2 v + (1 - beta2) g g;
 * p += -(lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps). */
int rg_adamw_step_sched(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                        long n, const rg_lr_schedule* sched, double beta1, double beta2,
                        double eps, double weight_decay, float grad_scale, const float* losses,
                        int n_losses,
                        int* step_state, int parity, void* stream);

/* ---------------------------------------------------------------- graph attention */

/* One nn.Linear of any width on the f32-input MFMA (exact f32 products; the chain kernels
 * and their packer stop at 256 features, the attention block's layers are up to 1024 wide):
 *   out[r][o] = act(sum_k in[r][k] weight[o][k] + bias[o]),  r < rows, o < out_dim.
 * weight: the float32 parameter where it lies, row-major [out_dim][ld_w] (no packed image);
 * bias float32 [out_dim] or NULL; act RG_ACT_*; rows_dev: optional device int32 row count
 * (`rows` is then the capacity).  Rows are independent of each other and of the launch
 * shape; each sum runs in ascending k.  ld_* in floats. */
int rg_linear_f32(const float* weight, int ld_w, const float* bias, int in_dim, int out_dim,
                  int act, const float* in, int ld_in, long rows, const int* rows_dev, float* out,
                  int ld_out, void* stream);

/* GATv2Conv(in, C, heads = H, edge_dim = Ce, concat = True, add_self_loops = False,
 * share_weights = False, bias = True), flow source -> target
 * (modules/neural_net/gnn/gnn_attention.py:26-36), forward only, float32, after the two node
 * projections:
 *   m_k   = xl[src[k]] + xr[i] + e_k W_e^T                     k in segment i, [H][C]
 *   a_kh  = sum_c att[h][c] leaky_relu(m_k[h][c], negative_slope)
 *   w_kh  = exp(a_kh - max_k' a_k'h) / (sum_k' exp(a_k'h - max) + 1e-16)   over segment i
 *   out_i = concat_h sum_k w_kh xl[src[k]][h][:] + bias                     [H C]
 * Two launches: the logits [E][H] (e W_e^T on v_mfma_f32_32x32x2_f32, one wave per head with
 * that head's W_e fragments in registers, the gathered rows as the accumulators' start), then
 * one wave per destination: the segment's maximum, then the weights and the weighted rows in
 * ascending edge position.  Nothing E x H C wide reaches memory, no atomics; a destination's
 * result does not depend on the rest of the batch or on the launch shape.  A destination
 * without incoming edges gets bias.
 *   xlr      float32 [n_nodes][ld_xlr]: xl = columns [0, H C), xr = columns [H C, 2 H C)
 *   e        float32 [n_edges_cap][ld_e], destination-major; positions from
 *            seg_ptr[n_nodes] up to n_edges_cap are never read (e, src, dst alike)
 *   seg_ptr  int32 [n_nodes + 1]; src, dst int32 [n_edges_cap]: the source and the owner of
 *            each position (out-of-range indices are clamped to [0, n_nodes))
 *   w_edge   lin_edge.weight where it lies, float32 [H C][ld_w]; att float32 [H C];
 *            bias float32 [H C]
 *   out      float32 [n_nodes][ld_out]
 * Rows (xlr, e, w_edge, att, out: base and stride) must be 16-byte aligned.  Compiled for
 * Ce = 64, C = 64, H = 8; any other shape: RG_ERR_UNSUPPORTED. */
size_t rg_gat_v2_layer_workspace_size(long n_edges_cap, int heads);
int rg_gat_v2_layer(const float* xlr, int ld_xlr, const float* e, int ld_e, const int* seg_ptr,
                    const int* src, const int* dst, int n_nodes, long n_edges_cap,
                    const float* w_edge, int ld_w, const float* att, const float* bias,
                    int edge_dim, int heads, int head_dim, float negative_slope, float* out,
                    int ld_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------- diagnostics */

/* Shader-clock calibration (bench.py; no product path calls it): n_blocks workgroups of
 * 256 threads, each wave one dependent chain of n_mfma (a multiple of 64)
 * v_mfma_f32_32x32x16_bf16 on register operands, stamped with s_memtime / s_memrealtime
 * around the chain.  out: device u64
 * [n_blocks][2] = (shader cycles, wall-clock ticks) of each workgroup's wave 0; sink: device
 * f32 [n_blocks * 4] (the chains' results); *wall_clock_khz_host = the wall-clock tick rate
 * (hipDeviceAttributeWallClockRate).  clock = cycles / ticks x rate. */
int rg_clock_probe(int n_blocks, int n_mfma, unsigned long long* out, float* sink,
                   int* wall_clock_khz_host, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* RADAR_GNN_H */
