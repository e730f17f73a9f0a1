/* tnc_hip — C ABI of the MI355X-native tensor-network contraction executor.
 *
 * This is the drop-in boundary. The reference delegates every
 * pairwise contraction to tblis::tensor_mult via
 *   TensorView::new(labels, shape, strides, ptr)  +
 *   tensor_mult(out_labels, out_shape, a, b) -> Vec<Complex64>
 * at tnc/src/tensornetwork/contraction.rs:111-113. tn_einsum_c128 exports the
 * same operation over complex128 buffers; tn_einsum_c128_dev is the
 * device-resident variant so the contraction walk never round-trips to host.
 * The tn_net_* entry points replace contract_tensor_network
 * (contraction.rs:35-68) for a flat replace-left plan.
 *
 * Conventions (matching the reference call site):
 *  - complex128, row-major unless strides say otherwise; strides are in
 *    ELEMENTS (ndarray-style, may describe non-contiguous views).
 *  - contracted labels = labels present in both A and B (never in out);
 *    out label set = symmetric difference, order chosen by the caller;
 *    K may be 1 (outer product); out may be rank 0 (scalar).
 *  - caller owns all buffers; out is caller-allocated with
 *    prod(out_shape) elements.
 *  - returns 0 on success, nonzero on error (tn_last_error() has the text).
 *    The reference unwraps/panics on error; callers should abort.
 *  - all compute requires an AMD GPU; there is no CPU fallback. Calls fail
 *    with TN_ERR_NO_GPU when no device is present.
 */

#ifndef TNC_HIP_H
#define TNC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  TN_OK = 0,
  TN_ERR_INVALID = 1,
  TN_ERR_NO_GPU = 2,
  TN_ERR_HIP = 3,
  TN_ERR_OOM = 4,
};

/* Last error message for this thread (valid until the next failing call). */
const char* tn_last_error(void);

/* Number of visible HIP devices (0 if the runtime reports none). */
int tn_device_count(void);

/* Synchronous einsum over HOST buffers (uploads, contracts on device 0 or
 * the device selected with tn_set_device, downloads). */
int tn_einsum_c128(const uint64_t* out_labels, const uint64_t* out_shape,
                   size_t out_ndim, const uint64_t* a_labels,
                   const uint64_t* a_shape, const int64_t* a_strides,
                   const void* a_data, size_t a_ndim, const uint64_t* b_labels,
                   const uint64_t* b_shape, const int64_t* b_strides,
                   const void* b_data, size_t b_ndim, void* out_data);

/* Einsum over DEVICE buffers, asynchronous on `stream` (a hipStream_t; NULL =
 * default stream). All pointers are device pointers on the current device.
 * Workspace (packing buffers) is drawn from the library's device pool. */
int tn_einsum_c128_dev(const uint64_t* out_labels, const uint64_t* out_shape,
                       size_t out_ndim, const uint64_t* a_labels,
                       const uint64_t* a_shape, const int64_t* a_strides,
                       const void* a_dev, size_t a_ndim,
                       const uint64_t* b_labels, const uint64_t* b_shape,
                       const int64_t* b_strides, const void* b_dev,
                       size_t b_ndim, void* out_dev, void* stream);

/* complex64 variants (the config-5 precision/throughput trade: f32 MFMA
 * runs at ~2x the f64 matrix rate). Same contract, 8-byte elements. */
int tn_einsum_c64(const uint64_t* out_labels, const uint64_t* out_shape,
                  size_t out_ndim, const uint64_t* a_labels,
                  const uint64_t* a_shape, const int64_t* a_strides,
                  const void* a_data, size_t a_ndim, const uint64_t* b_labels,
                  const uint64_t* b_shape, const int64_t* b_strides,
                  const void* b_data, size_t b_ndim, void* out_data);

int tn_einsum_c64_dev(const uint64_t* out_labels, const uint64_t* out_shape,
                      size_t out_ndim, const uint64_t* a_labels,
                      const uint64_t* a_shape, const int64_t* a_strides,
                      const void* a_dev, size_t a_ndim,
                      const uint64_t* b_labels, const uint64_t* b_shape,
                      const int64_t* b_strides, const void* b_dev,
                      size_t b_ndim, void* out_dev, void* stream);

/* Select the HIP device used by subsequently created nets / einsum calls. */
int tn_set_device(int device);

/* ------------------------- step planner ------------------------------ */

enum { TN_ROUTE_DOT = 0, TN_ROUTE_GATHER = 1, TN_ROUTE_TTGT = 2 };
enum { TN_DOT_LINEAR = 0, TN_DOT_TILED = 1, TN_DOT_GATHER = 2 };
enum {
  TN_GEMM_V1 = 0,          /* LDS-tiled VALU GEMM, ragged / small shapes */
  TN_GEMM_MFMA = 1,        /* generic MFMA GEMM (c64 with ragged edges) */
  TN_GEMM_C128_GLDS = 2,   /* c128 MFMA, ragged edges */
  TN_GEMM_C128_PURE = 3,   /* c128 MFMA, M%128 == N%64 == K%16 == 0 */
  TN_GEMM_C128_3M = 4,     /* c128 Gauss three-multiply MFMA */
  TN_GEMM_C128_GATHER = 5, /* c128 MFMA reading through the pack permute */
  TN_GEMM_C64_PURE = 6,    /* c64 MFMA, pure shapes */
};
/* The gather-route kernels. P2 / TBL: every axis of the out map and of the K
 * map is a power of two, indices decode by shift and mask; otherwise by
 * division and remainder. */
enum {
  TN_GK_NONE = 0,
  TN_GK_SMALLK = 1,     /* k_einsum_smallk<false>: K <= 64, offsets in LDS */
  TN_GK_SMALLK_P2 = 2,  /* k_einsum_smallk<true> */
  TN_GK_SMALLK_TBL = 3, /* k_einsum_smallk_tbl: 2^26 <= out elements < 2^32,
                         * rank >= 8, four 8-bit offset tables, grid capped
                         * at 32768 blocks */
  TN_GK_ANYK = 4,       /* k_einsum_anyk<false>: K > 64 */
  TN_GK_ANYK_P2 = 5,    /* k_einsum_anyk<true> */
};

/* How one einsum step is dispatched: everything that follows from dtype,
 * shapes, strides and the TN_* environment switches alone. What depends on
 * an allocation failing at run time (split-K dropping to 1, the pipeline
 * dropping to the serial pack, out-of-memory dropping to the gather route)
 * is not in here. */
typedef struct tn_step_plan {
  uint64_t m, n, k;
  int32_t route;    /* TN_ROUTE_* */
  int32_t kind;     /* as tn_net_contract_profiled reports it:
                     * 0 gather, 1 dot, 5 linear dot, 6 tiled dot,
                     * 2 TTGT, 3 TTGT with out permute */
  int32_t dot_form; /* TN_DOT_* (dot route) */
  int32_t tbits;    /* tiled dot: bits left to the grid */
  uint64_t dot_blocks; /* dot route: partial-sum blocks */
  int32_t gather_ok;   /* TTGT may drop to the gather route on out-of-memory */
  int32_t pack_a, pack_b; /* operand is not already in [M][K] / [K][N] order
                           * (reported on every route) */
  int32_t direct;      /* GEMM writes `out` without a final permute */
  int32_t gather_gemm; /* packs folded into the GEMM's staging */
  /* pack pipeline: pipe_p K-windows of pipe_kc over the first pipe_npre K
   * legs of A; 0 = serial pack */
  int32_t pipe_p, pipe_npre;
  uint64_t pipe_kc;
  /* GEMM of the serial path */
  uint64_t row_tiles, col_tiles, splitk, kchunk;
  int32_t kernel; /* TN_GEMM_* */
  /* workspace bytes the step will ask for. A pipelined step holds its window
   * buffers in ws_pack_a / ws_pack_b and has no split buffer. */
  uint64_t ws_pack_a, ws_pack_b, ws_tmp_c, ws_slices, ws_split, ws_dot;
  /* a non-direct out order is stored by the GEMM's scatter epilogue: no
   * temporary C (ws_tmp_c == 0), no out permute (kind 2) */
  int32_t scatter_out;
  /* the 3M kernel runs its pipelined main loop (TN_GEMM3M_PIPE) */
  int32_t gemm_pipe;
  /* the permute kernel of each pack / unpack: 0 none, 1 k_permute_ct (index
   * gather), 2 k_permute_tile (tiled bit permutation). perm_a / perm_b /
   * perm_out: the serial path's pack of A, pack of B and out permute.
   * pipe_perm_a / pipe_perm_b: the window permutes of a pipelined step (0
   * when pipe_p == 0; pipe_perm_b is 0 when B is ready). */
  int32_t perm_a, perm_b, perm_out;
  int32_t pipe_perm_a, pipe_perm_b;
  /* the gather kernel (TN_GK_*) and its grid, in blocks of 256 threads:
   * what the step launches on the gather route, and what a TTGT step with
   * gather_ok launches when it drops there on out-of-memory. TN_GK_NONE and
   * 0 on the dot route and on TTGT steps without gather_ok. */
  int32_t gather_kernel;
  int32_t gather_blocks;
} tn_step_plan;

/* Plan the step tn_einsum_*_dev would run on these operands (dtype 0 =
 * complex128, 1 = complex64; has_stream2 = a second stream is available for
 * the pack pipeline, as inside a tn_net). Needs no GPU and touches none.
 * NULL strides mean contiguous row-major. Returns TN_ERR_INVALID, with the
 * text in tn_last_error, for operands the einsum would reject. */
int tn_plan_step(int dtype, const uint64_t* out_labels,
                 const uint64_t* out_shape, size_t out_ndim,
                 const uint64_t* a_labels, const uint64_t* a_shape,
                 const int64_t* a_strides, size_t a_ndim,
                 const uint64_t* b_labels, const uint64_t* b_shape,
                 const int64_t* b_strides, size_t b_ndim, int has_stream2,
                 tn_step_plan* plan);

/* The layout pre-pass the network executor runs before its walk: for a flat
 * replace-left path over leaves given as concatenated labels/dims (leaf_nd
 * entries each), decide the order every step stores its output in. A step
 * whose consumer would pack that output stores it in the consumer's operand
 * layout instead, when the scatter epilogue can write it (scatter_out[s] =
 * 1). inline_pack_bytes[s] is what step s still packs inline, on the main
 * stream: operands that are not in GEMM layout and could not be prepacked
 * during the previous step because that step produces them. Either output
 * may be NULL. Needs no GPU; honours TN_EPI_SCATTER. */
int tn_plan_layouts(int dtype, const uint64_t* leaf_labels,
                    const uint64_t* leaf_dims, const uint64_t* leaf_nd,
                    size_t nleaves, const uint64_t* pairs, size_t nsteps,
                    int32_t* scatter_out, uint64_t* inline_pack_bytes);

/* The slice plan of tn_net_contract_sliced: leaves and path as for
 * tn_plan_layouts, plus the labels to fix. *nassign gets the number of
 * assignments (the product of the labels' dims); assignment index t decodes
 * with the first label most significant, the order of a nested loop with the
 * first label outermost. reduced_nd[nleaves] gets each leaf's rank with the
 * slice labels removed, strides[nleaves * nlabels] (row-major) the element
 * stride of each slice label in each stored leaf, 0 where the leaf does not
 * carry it: the flat offset of assignment t in a leaf is the sum over labels
 * of digit * stride. Any output may be NULL. Returns TN_ERR_INVALID, with the
 * text in tn_last_error, when a label is in no leaf, is listed twice, is
 * carried by a number of leaves other than two or is a leg of the final
 * tensor, when the assignment count overflows 64 bits, and for a path
 * tn_plan_layouts refuses. Needs no GPU. */
int tn_plan_slices(int dtype, const uint64_t* leaf_labels,
                   const uint64_t* leaf_dims, const uint64_t* leaf_nd,
                   size_t nleaves, const uint64_t* pairs, size_t nsteps,
                   const uint64_t* slice_labels, size_t nlabels,
                   uint64_t* nassign, uint64_t* reduced_nd,
                   uint64_t* strides);

/* --------------------------- batch labels ----------------------------- */

/* A batch label is carried by both operands of a step AND kept in out, not
 * summed: out[b.., m.., n..] = sum_k A[b.., m.., k..] * B[b.., k.., n..].
 * The caller lists the labels that may act so (batch_labels). A listed label
 * found in both operands is a step-batch label: it must appear in out with
 * the same dim, and the step-batch labels must be the leading axes of out
 * (any order among themselves), so one batch element of out is contiguous. A
 * listed label found in one operand only is an ordinary free label; a label
 * in both operands that is not listed is contracted, as everywhere else. */
enum { TN_BATCH_NONE = 0, TN_BATCH_GATHER = 1, TN_BATCH_GEMM = 2,
       TN_BATCH_LOOP = 3 };

typedef struct tn_batch_plan {
  uint64_t batch;       /* product of the step-batch dims; 1 = none */
  int32_t cls;          /* TN_BATCH_* */
  uint64_t dispatches;  /* compute dispatches: 1 for GATHER/GEMM, batch for LOOP */
  uint64_t ws_pack_a, ws_pack_b; /* batched pack buffers (GEMM class), 0 if ready */
  tn_step_plan elem;    /* plan of one batch element (whole step when NONE) */
  /* class GATHER: the kernel (TN_GK_*) of the one launch over all of out,
   * the batch axes counted into its out map (a batch dim that is no power of
   * two makes it a div/mod kernel whatever elem.gather_kernel says). 0 for
   * the other classes. */
  int32_t gather_kernel;
} tn_batch_plan;

/* Plan the step tn_einsum_*_batched_dev would run. Arguments as tn_plan_step
 * plus the batch labels. TN_BATCH_NONE: no step-batch label, elem is
 * tn_plan_step's plan of the same operands. TN_BATCH_GATHER: the element is on
 * the gather route; one launch of the gather kernels covers all of out.
 * TN_BATCH_GEMM: the element is an unsplit TTGT GEMM of fewer than 256 tiles;
 * operands are packed to [batch][M][K] / [batch][K][N] where they are not in
 * that order already and one launch of the batched MFMA kernel computes every
 * element (TN_BATCH_GEMM=0 in the environment turns this class into LOOP).
 * TN_BATCH_LOOP: the element step runs `batch` times on offset views. Needs
 * no GPU. */
int tn_plan_step_batched(int dtype, const uint64_t* out_labels,
                         const uint64_t* out_shape, size_t out_ndim,
                         const uint64_t* a_labels, const uint64_t* a_shape,
                         const int64_t* a_strides, size_t a_ndim,
                         const uint64_t* b_labels, const uint64_t* b_shape,
                         const int64_t* b_strides, size_t b_ndim,
                         const uint64_t* batch_labels, size_t nbatch,
                         int has_stream2, tn_batch_plan* plan);

/* The walk plan of tn_net_contract_batched: leaves and path as for
 * tn_plan_layouts, plus the batch labels. Step s stores its output as
 * [batch labels carried by both operands, in batch_labels order][A-only legs
 * in A order][B-only legs in B order]. cls[nsteps] gets each step's
 * TN_BATCH_* class, out_nd[nsteps] the rank of its output, out_labels
 * (nsteps rows of 64) the labels in stored order, ws_bytes[nsteps] the
 * workspace the step asks for beyond its output. Any output may be NULL.
 * Returns TN_ERR_INVALID, with the text in tn_last_error, for a path or rank
 * tn_plan_layouts refuses and for a batch label that is listed twice, is in
 * no leaf or has differing dims across leaves. Needs no GPU. */
int tn_plan_batch_walk(int dtype, const uint64_t* leaf_labels,
                       const uint64_t* leaf_dims, const uint64_t* leaf_nd,
                       size_t nleaves, const uint64_t* pairs, size_t nsteps,
                       const uint64_t* batch_labels, size_t nbatch,
                       int32_t* cls, uint64_t* out_nd, uint64_t* out_labels,
                       uint64_t* ws_bytes);

/* Batched einsum: tn_einsum_* with batch labels (semantics above). */
int tn_einsum_c128_batched(const uint64_t* out_labels,
                           const uint64_t* out_shape, size_t out_ndim,
                           const uint64_t* a_labels, const uint64_t* a_shape,
                           const int64_t* a_strides, const void* a_data,
                           size_t a_ndim, const uint64_t* b_labels,
                           const uint64_t* b_shape, const int64_t* b_strides,
                           const void* b_data, size_t b_ndim,
                           const uint64_t* batch_labels, size_t nbatch,
                           void* out_data);

int tn_einsum_c64_batched(const uint64_t* out_labels,
                          const uint64_t* out_shape, size_t out_ndim,
                          const uint64_t* a_labels, const uint64_t* a_shape,
                          const int64_t* a_strides, const void* a_data,
                          size_t a_ndim, const uint64_t* b_labels,
                          const uint64_t* b_shape, const int64_t* b_strides,
                          const void* b_data, size_t b_ndim,
                          const uint64_t* batch_labels, size_t nbatch,
                          void* out_data);

int tn_einsum_c128_batched_dev(const uint64_t* out_labels,
                               const uint64_t* out_shape, size_t out_ndim,
                               const uint64_t* a_labels,
                               const uint64_t* a_shape,
                               const int64_t* a_strides, const void* a_dev,
                               size_t a_ndim, const uint64_t* b_labels,
                               const uint64_t* b_shape,
                               const int64_t* b_strides, const void* b_dev,
                               size_t b_ndim, const uint64_t* batch_labels,
                               size_t nbatch, void* out_dev, void* stream);

int tn_einsum_c64_batched_dev(const uint64_t* out_labels,
                              const uint64_t* out_shape, size_t out_ndim,
                              const uint64_t* a_labels,
                              const uint64_t* a_shape,
                              const int64_t* a_strides, const void* a_dev,
                              size_t a_ndim, const uint64_t* b_labels,
                              const uint64_t* b_shape,
                              const int64_t* b_strides, const void* b_dev,
                              size_t b_ndim, const uint64_t* batch_labels,
                              size_t nbatch, void* out_dev, void* stream);

/* ------------ network executor (contract_tensor_network) ------------- */

typedef struct tn_net tn_net;

/* Create an executor bound to `device` (complex128 tensors). */
tn_net* tn_net_create(int device);

/* Like tn_net_create with an element type: dtype 0 = complex128,
 * 1 = complex64 (leaf/result buffers are then 8-byte elements). */
tn_net* tn_net_create2(int device, int dtype);

/* Reserve a device arena of `bytes` for intermediates and packing
 * workspaces (one hipMalloc; first-fit, stream-ordered reuse). Without a
 * reservation the executor falls back to stream-ordered hipMallocAsync,
 * which costs seconds per contraction at tens-of-GB intermediates. */
int tn_net_reserve(tn_net* net, uint64_t bytes);

/* Register leaf `index = return value` with labels/dims and host data
 * (complex128, row-major, contiguous). Data is uploaded immediately and
 * persists across contract calls. Returns a negative value on error. */
int64_t tn_net_add_leaf(tn_net* net, const uint64_t* labels,
                        const uint64_t* dims, size_t ndim,
                        const void* host_data);

/* Contract along a flat replace-left path: pairs = [i0,j0, i1,j1, ...].
 * Equivalent to the reference's recursive walk after flattening
 * (contraction.rs:35-68). Intermediates stay on device; leaves are not
 * consumed, so the call is repeatable. Synchronizes before returning;
 * elapsed_ms (optional) gets the device-side wall time of the walk. */
int tn_net_contract(tn_net* net, const uint64_t* pairs, size_t nsteps,
                    double* elapsed_ms);

/* Like tn_net_contract but also fills per-step kernel timings:
 * step_ms[nsteps] = HIP-event time of step s (all kernels of the step),
 * gemm_ms[nsteps] = time of the GEMM kernel alone (0 for non-GEMM steps),
 * kind[nsteps] = kernel class (0=smallk stream, 1=dot, 2=gemm+packs,
 * 3 = gemm with unpack). */
int tn_net_contract_profiled(tn_net* net, const uint64_t* pairs, size_t nsteps,
                             double* step_ms, double* gemm_ms, int32_t* kind,
                             double* elapsed_ms);

/* Contract the network as the sum, over the listed assignments of the slice
 * labels, of the network with those labels fixed. Same path for every
 * assignment. which[nwhich] are assignment indices (first label most
 * significant); the result (tn_net_result_*) is the sum in that order.
 * nlabels == 0 with which = {0} is the plain contraction.
 * The leaves stay as uploaded: each assignment gathers the leaves that carry
 * a slice label into per-net shadow buffers on the device, walks the path as
 * a net holding the reduced leaves would, and adds its final tensor to an
 * accumulator, all on the net's stream without a host wait in between.
 * elapsed_ms (optional) gets the device time of all assignments. Returns
 * TN_ERR_INVALID, with nothing launched, for a slice plan tn_plan_slices
 * refuses, an index at or beyond the assignment count, and nwhich == 0. */
int tn_net_contract_sliced(tn_net* net, const uint64_t* pairs, size_t nsteps,
                           const uint64_t* slice_labels, size_t nlabels,
                           const uint64_t* which, size_t nwhich,
                           double* elapsed_ms);

/* Contract along the path keeping the listed batch labels: a label of
 * batch_labels carried by several leaves is never summed, and the final
 * tensor keeps it (one amplitude per bitstring when the bras are [B, 2]
 * leaves sharing one label). Stored orders and step classes are those of
 * tn_plan_batch_walk; there is no look-ahead pack, no scatter epilogue and
 * no hipGraph capture in this walk. The walk plan and the captured graph
 * tn_net_contract keeps for the net are left as they are, so the two calls
 * may alternate on one net. nbatch == 0 gives the final tensor of
 * tn_net_contract. Results are read with tn_net_result_*. */
int tn_net_contract_batched(tn_net* net, const uint64_t* pairs, size_t nsteps,
                            const uint64_t* batch_labels, size_t nbatch,
                            double* elapsed_ms);

/* Synchronous device-to-device copy on the current device (for exchanging
 * buffers with an external allocator, e.g. RCCL-communicated tensors). */
int tn_memcpy_dtod(void* dst, const void* src, uint64_t bytes);

/* Synchronous device-to-host copy (fetch an exchanged intermediate). */
int tn_memcpy_dtoh(void* host_dst, const void* dev_src, uint64_t bytes);

/* Metadata of the final tensor after the last contract call. labels/dims
 * must have room for 64 entries. */
int tn_net_result_meta(tn_net* net, uint64_t* labels, uint64_t* dims,
                       size_t* ndim);

/* Copy the final tensor to host (caller-allocated, prod(dims) c128). */
int tn_net_result_data(tn_net* net, void* host_out);

/* Device pointer of the final tensor (valid until the next contract call). */
void* tn_net_result_dev(tn_net* net);

/* ------------------- sampling a tensor's |amplitude|^2 ------------------ */

/* Draw flat indices of a contiguous complex tensor T[n] with probability
 * |T[i]|^2 / sum |T|^2, from uniforms the caller supplies (0 <= u < 1; the
 * library owns no random generator). Fixed semantics (DESIGN.md "Sampling
 * the final tensor"): p[i] = re^2 + im^2 in f64; chunks of 4096 elements;
 * S[j] the sum of p over chunk j; C the inclusive prefix of S, added one
 * after another in ascending j; total = C[last]; t = u * total. The chunk is
 * the first j with C[j] > t, else the last chunk that added mass; the element
 * is the first of the chunk whose running sum exceeds t - C[j-1], else the
 * chunk's last element with p > 0. No atomics: two runs give the same bits.
 * An element with p == 0 is never drawn. */
typedef struct tn_sample_plan {
  uint64_t chunk;      /* elements per chunk (4096) */
  uint64_t nchunks;
  uint64_t grid_sums;  /* blocks of k_prob_chunk_sums: one per chunk */
  uint64_t grid_scan;  /* blocks of k_prob_scan: 1 */
  uint64_t grid_draw;  /* blocks of k_sample_draw: one per shot (0: no launch) */
  /* workspace of tn_net_sample: nchunks doubles (C), nshots doubles (u),
   * nshots uint64 (idx), one double (total). tn_sample_*_dev use only the
   * first nchunks doubles. */
  uint64_t ws_bytes;
} tn_sample_plan;

/* Plan the three launches. dtype 0 = complex128, 1 = complex64. Returns
 * TN_ERR_INVALID for n == 0 and for more chunks or shots than one grid holds
 * (2^31 - 1). Needs no GPU. */
int tn_plan_sample(uint64_t n, uint64_t nshots, int dtype,
                   tn_sample_plan* out);

/* Sample a device tensor: data (n elements, contiguous, 16-byte aligned),
 * u_dev[nshots], idx_dev[nshots], norm2_dev[1] and ws_dev are device
 * pointers; ws_bytes must cover nchunks doubles (tn_plan_sample's ws_bytes
 * always does). Launches on `stream` and returns without waiting; *norm2_dev
 * receives total, which the caller checks: where it is zero or not finite
 * the indices mean nothing (they stay inside [0, n)). u outside [0, 1) is not
 * detected here. nshots == 0 computes total only. */
int tn_sample_c128_dev(const void* data, uint64_t n, const double* u_dev,
                       uint64_t nshots, uint64_t* idx_dev, double* norm2_dev,
                       void* ws_dev, uint64_t ws_bytes, void* stream);
int tn_sample_c64_dev(const void* data, uint64_t n, const double* u_dev,
                      uint64_t nshots, uint64_t* idx_dev, double* norm2_dev,
                      void* ws_dev, uint64_t ws_bytes, void* stream);

/* Sample the net's final tensor (after any tn_net_contract* call), in its
 * stored order (tn_net_result_meta). Host arrays in and out, synchronous.
 * idx_host[s] is the flat index drawn for u_host[s]; *norm2 (optional) gets
 * total. Workspace comes from the net's arena when there is one, else from
 * hipMalloc, and is released before the call returns: the arena stands as it
 * did and a captured graph of tn_net_contract stays valid. Returns
 * TN_ERR_INVALID with nothing launched when there is no final tensor, it has
 * no elements, or a u is outside [0, 1); after the first two launches, when
 * total is zero ("final tensor has zero norm") or not finite ("final tensor
 * norm is not finite"). nshots == 0 gives *norm2 only. */
int tn_net_sample(tn_net* net, const double* u_host, uint64_t nshots,
                  uint64_t* idx_host, double* norm2);

/* Import an external DEVICE tensor (e.g. an RCCL-received intermediate) as a
 * new leaf without copying; the buffer must outlive the net or be detached
 * before reuse. The contents of the buffer may change between contract calls
 * (a receive landing in the same buffer every round): every tn_net_contract*
 * call reads them as they are when the call is made, whether it walks
 * normally, captures a graph or replays one, since a captured graph reads
 * through this pointer. The pointer, the labels and the dims may not
 * change. */
int64_t tn_net_add_leaf_dev(tn_net* net, const uint64_t* labels,
                            const uint64_t* dims, size_t ndim, void* dev_data);

/* Bytes currently held by the net's device pool (watermark telemetry). */
int tn_net_pool_bytes(tn_net* net, uint64_t* in_use, uint64_t* cached);

/* Replay telemetry: *plain gets the state of tn_net_contract's graph, *sliced
 * that of tn_net_contract_sliced's (0 when there is no slice state):
 * 0 nothing armed, 1 armed (the next identical call captures), 2 captured
 * (identical calls replay), -1 disabled after a spill or failure. Either may
 * be NULL. */
int tn_net_replay_state(tn_net* net, int32_t* plain, int32_t* sliced);

void tn_net_destroy(tn_net* net);

#ifdef __cplusplus
}
#endif

#endif /* TNC_HIP_H */
