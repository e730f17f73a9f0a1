// step_plan.hpp — the one place a contraction step's dispatch is decided.
//
// plan_step() maps (dtype, out order, operand shapes/strides, environment) to
// a StepPlan: route (dot / gather / TTGT), which operands get packed, the
// pack-pipeline windows, split-K, the GEMM kernel, the permute kernel of
// every pack and unpack (plan_permute_tile: k_permute_tile or k_permute_ct,
// over the axis lists the executor launches with), the gather kernel and its
// grid (plan_gather_kernel, likewise) and the workspace the step will ask
// for. No HIP call, no HIP header: it builds with a plain host
// compiler and runs without a GPU. The executor (einsum_dev_impl), the walk
// plan of a whole path (plan_layouts, below: stored orders and look-ahead
// packs) and the Python arena model (through tn_plan_step) all read this
// plan; none re-derives it. plan_slices (at the end) is the same for edge
// slicing: reduced leaves, per-leaf offsets and the walk plan of one slice,
// read by tn_net_contract_sliced and through tn_plan_slices. Only what
// depends on
// an allocation failing at run time stays in the executor: split-K falling
// back to 1, the pipeline to the serial pack, out-of-memory to the gather
// route.

#ifndef TNC_STEP_PLAN_HPP
#define TNC_STEP_PLAN_HPP

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tnc_hip.h"

typedef uint64_t u64;
typedef int64_t i64;

// ---- tile constants shared by the kernels and the planner -----------------

#define TN_MAXR 40   // max axes per map
#define TN_SMALLK 64 // LDS-precomputed K offsets

// k_dot_tile: 6 a-bits (lane index) + 6 b-bits per block, the rest one block
// per combination
#define TN_DOT_TILE_ABITS 6
#define TN_DOT_TILE_BBITS 6
#define TN_DOT_TILE_BITS (TN_DOT_TILE_ABITS + TN_DOT_TILE_BBITS)
#define TN_DOT_MAXBITS 34

// k_permute_tile: 6 a-bits (lane index of the coalesced read) + 5 b-bits
// (lane index of the coalesced write) per block, the rest one block per
// combination.
#define TN_PERM_AB 6
// BB=5 (64x32 tiles, 32 KB LDS -> more blocks/CU) measured 5.2 TB/s vs
// 4.3 TB/s at 6/6 on the rqc36-interleave shape and holds 5.2 on bit
// reversal (scripts/perm_tune.hip scan, r02)
#define TN_PERM_BB 5
#define TN_PERM_MAXBITS 34

#define GT 64        // k_zgemm_v1 tile edge; column-tile width of every GEMM
#define MF_T 128      // MFMA tile rows = MF_WAVES * 16
#define MF_TN 64      // MFMA tile cols
#define MF_K 16

// ---- plain-data kernel arguments the planner fills ------------------------

struct DotPerm {
  int rbits;
  u64 restA[TN_DOT_MAXBITS];  // element strides of each rest bit
  u64 restB[TN_DOT_MAXBITS];
  u64 bA[TN_DOT_TILE_BBITS];  // A strides of the b-bits
  u64 bB[TN_DOT_TILE_BBITS];  // B strides of the b-bits (ascending)
  u64 aB[TN_DOT_TILE_ABITS];  // B strides of the a-bits (A strides are 1<<i)
};

struct PermPerm {
  int rbits;
  u64 restS[TN_PERM_MAXBITS];  // src / dst element strides of each rest bit
  u64 restD[TN_PERM_MAXBITS];
  u64 bS[TN_PERM_BB];  // src strides of the b-bits
  u64 bD[TN_PERM_BB];  // dst strides of the b-bits (ascending)
  u64 aD[TN_PERM_AB];  // dst strides of the a-bits (src strides are 1<<i)
};

struct GatherGemmMap {
  int rbits, kbits;  // bits of the row index (M for A / N for B) and of k
  u64 rstride[34];    // source stride (elements) contributed by row bit b
  u64 kstride[34];    // source stride contributed by k bit b
};

// Scatter epilogue: C(row, col) is stored at out[R(row) + Cc(col)]. With
// every out dim a power of two each destination index bit comes from one row
// bit or one column bit, so the offset is separable.
#define TN_SCATTER_MINRUN 3  // low column bits that must stay in place
struct ScatterMap {
  int rbits, cbits;   // bits of the row (M) and column (N) index
  u64 rstride[34];    // destination stride (elements) of row bit b
  u64 cstride[34];    // destination stride of column bit b
};

struct Meta {
  int nd;
  u64 labels[TN_MAXR];
  u64 dims[TN_MAXR];
  i64 strides[TN_MAXR];  // in elements
  const void* data;
};

struct AxisInfo {
  u64 dim;
  i64 sa;
  i64 sb;
};

// fixed-capacity axis list (a step plans without touching the heap)
struct AxisList {
  int n = 0;
  int v[TN_MAXR];
  void push_back(int x) { v[n++] = x; }
  bool empty() const { return n == 0; }
  int operator[](int i) const { return v[i]; }
  int front() const { return v[0]; }
  int back() const { return v[n - 1]; }
  const int* begin() const { return v; }
  const int* end() const { return v + n; }
};

// ---- gather maps ----------------------------------------------------------
// A packed row-major index p over an axis list (outer..inner) decodes to one
// coordinate per axis; the source offsets are the sums of coordinate times
// stride. Two ENCODINGS of the decode, chosen per launch:
//   div/mod     c_i = (p / pstride[i]) % dim[i]   pstride = suffix product
//   shift/mask  c_i = (p >> pstride[i]) & dim[i]  pstride = log2 of it,
//               (every dim a power of two)        dim = dim - 1
struct GatherMap {
  int n;
  int pow2;             // if set: pstride holds shifts, dim holds masks
  u64 pstride[TN_MAXR]; // packed-linear stride (suffix product) or shift
  u64 dim[TN_MAXR];     // axis dim, or mask (dim-1) when pow2
  i64 sa[TN_MAXR];      // source-A stride in elements (0 if absent)
  i64 sb[TN_MAXR];      // source-B stride in elements
};

inline int log2_u64(u64 v) {
  int s = 0;
  while ((1ull << s) < v) ++s;
  return s;
}

inline bool axes_pow2(const std::vector<AxisInfo>& axes) {
  for (const auto& a : axes)
    if (a.dim & (a.dim - 1)) return false;
  return true;
}

// Encode a map. The pow2 (shift/mask) and general (div/mod) ENCODINGS are
// incompatible; when a kernel takes several maps the caller must pick ONE
// encoding for all of them (allow_pow2 = the joint decision).
inline int build_map(const std::vector<AxisInfo>& axes, GatherMap* m,
                     bool allow_pow2 = true) {
  int n = (int)axes.size();
  if (n > TN_MAXR) return -1;
  m->n = n;
  u64 pstride = 1;
  bool p2 = allow_pow2 && axes_pow2(axes);
  for (int i = n - 1; i >= 0; --i) {
    m->pstride[i] = pstride;
    m->dim[i] = axes[i].dim;
    m->sa[i] = axes[i].sa;
    m->sb[i] = axes[i].sb;
    pstride *= axes[i].dim;
  }
  m->pow2 = p2 ? 1 : 0;
  if (p2) {
    for (int i = 0; i < n; ++i) {
      m->pstride[i] = (u64)log2_u64(m->pstride[i]);
      m->dim[i] = m->dim[i] - 1;
    }
  }
  return 0;
}

// ---- environment switches, each read once on first use --------------------
//   TN_NO_PIPELINE    set: never use the pack pipeline
//   TN_PIPELINE_FORCE set: pipeline every shape-feasible step, profitability
//                     gate ignored (tests: runs the window/event machinery
//                     on small cases)
//   TN_GATHER_GEMM    set: allow the gather-staged GEMM. OPT-IN: on the rqc36
//                     dominant shapes it is ~35% SLOWER than pack + pure GEMM
//                     (44.9 vs 69.6 TF/s on M16384/N4096/K32768), because the
//                     GEMM re-reads its operand strips ~12x across tiles —
//                     the pack is a bandwidth AMORTIZER, not removable
//                     overhead. Kept for low-reuse shapes and as a recorded
//                     negative result.
//   TN_GEMM3M         unset: Gauss 3M kernel where the profitability gate
//                     admits the shape; "0": never (the 4M-only dispatch);
//                     "force": wherever the kernel's structural preconditions
//                     hold, gate ignored (tests; also lets split-K slices
//                     run through it, which the default never does)
//   TN_GEMM3M_PIPE    unset: the 3M kernel runs its pipelined main loop
//                     (operand staging of the next K-slab under the MFMAs of
//                     this one); "0": the serial loop (stage, barrier, MFMAs,
//                     barrier), same binary, bit-identical results
//   TN_NO_PREPACK     set: no look-ahead pack of the next step's operands
//   TN_EPI_SCATTER    unset: the 3M GEMM may store its output through the
//                     scatter epilogue, and plan_layouts may choose a step's
//                     stored order for its consumer; "0": neither (every
//                     step stores the symmetric-difference order)
//   TN_BATCH_GEMM     unset: a batched step whose element is a small unsplit
//                     GEMM runs as one launch of k_zgemm_batched; "0": it
//                     loops over the batch elements instead (TN_BATCH_LOOP),
//                     the A/B handle of scripts/batch_amplitudes.py
enum EnvSwitch { ENV_NO_PIPELINE, ENV_PIPELINE_FORCE, ENV_GATHER_GEMM,
                 ENV_GEMM3M, ENV_NO_PREPACK, ENV_EPI_SCATTER, ENV_GEMM3M_PIPE,
                 ENV_BATCH_GEMM, ENV_COUNT };
enum { GEMM3M_OFF = 0, GEMM3M_GATED = 1, GEMM3M_FORCE = 2 };

inline int env_switch(EnvSwitch s) {
  static const char* const names[ENV_COUNT] = {
      "TN_NO_PIPELINE", "TN_PIPELINE_FORCE", "TN_GATHER_GEMM", "TN_GEMM3M",
      "TN_NO_PREPACK", "TN_EPI_SCATTER", "TN_GEMM3M_PIPE", "TN_BATCH_GEMM"};
  static int cache[ENV_COUNT] = {-1, -1, -1, -1, -1, -1, -1, -1};
  int& v = cache[s];
  if (v < 0) {
    const char* e = getenv(names[s]);
    const bool on = e && e[0] && e[0] != '0';
    if (s == ENV_EPI_SCATTER || s == ENV_GEMM3M_PIPE || s == ENV_BATCH_GEMM)
      v = (!e || !e[0] || on) ? 1 : 0;  // on unless "0"
    else if (s != ENV_GEMM3M)
      v = on ? 1 : 0;
    else if (!e || !e[0])
      v = GEMM3M_GATED;
    else
      v = !strcmp(e, "force") ? GEMM3M_FORCE : on ? GEMM3M_GATED : GEMM3M_OFF;
  }
  return v;
}

// The plan: the exported scalars (tn_step_plan, include/tnc_hip.h) plus what
// only the executor needs, the axis lists and the kernel-argument maps.
struct StepPlan : tn_step_plan {
  int apos[TN_MAXR], bpos[TN_MAXR];  // position in A / B of each out axis
  AxisList m_out, n_out;             // positions (in out) of M legs / N legs
  AxisList k_a, k_b;                 // K legs, A order: axes in A / in B
  // GEMM operand layouts: A' = [M legs in out order][K legs in A order],
  // B' = [K legs in A order][N legs in out order]
  AxisList a_axes, b_axes;
  DotPerm dp;              // dot route, tiled form
  GatherGemmMap gmA{}, gmB{};  // TTGT route, gather_gemm
  ScatterMap smap{};           // TTGT route, scatter_out
  u64 nout() const { return m * n; }
};

inline int grid_for(u64 nout, int block = 256) {
  u64 blocks = (nout + (u64)block - 1) / block;
  u64 cap = 64 * 2048;  // grid-stride covers the remainder
  if (blocks > cap) blocks = cap;
  if (blocks == 0) blocks = 1;
  return (int)blocks;
}

// The axis lists of a gather launch. plan_step (gather_kernel) and run_gather
// (the launch) both build them here.
// Out map: `lead` (a batched step's batch axes, which carry a stride in BOTH
// operands), then every out axis with its source stride in A or B.
inline std::vector<AxisInfo> gather_out_axis_info(
    const StepPlan& p, const u64* out_shape, int out_nd, const Meta& A,
    const Meta& B, const std::vector<AxisInfo>& lead = {}) {
  std::vector<AxisInfo> oax;
  oax.reserve(lead.size() + out_nd);
  oax.assign(lead.begin(), lead.end());
  for (int i = 0; i < out_nd; ++i) {
    AxisInfo ax;
    ax.dim = out_shape[i];
    ax.sa = p.apos[i] >= 0 ? A.strides[p.apos[i]] : 0;
    ax.sb = p.bpos[i] >= 0 ? B.strides[p.bpos[i]] : 0;
    oax.push_back(ax);
  }
  return oax;
}

// K axes with their strides in A and B
inline std::vector<AxisInfo> k_axis_info(const StepPlan& p, const Meta& A,
                                         const Meta& B) {
  std::vector<AxisInfo> kax;
  kax.reserve(p.k_a.n + 1);
  for (int t = 0; t < p.k_a.n; ++t)
    kax.push_back(
        {A.dims[p.k_a[t]], A.strides[p.k_a[t]], B.strides[p.k_b[t]]});
  return kax;
}

// K map of a gather launch: never empty (K = 1 decodes one axis of 1)
inline std::vector<AxisInfo> gather_k_axis_info(const StepPlan& p,
                                                const Meta& A, const Meta& B) {
  std::vector<AxisInfo> kax = k_axis_info(p, A, B);
  if (kax.empty()) kax.push_back({1, 0, 0});
  return kax;
}

// Which gather kernel run_gather launches (TN_GK_*), on how many blocks of
// 256 threads, and the one encoding both maps take. pow2 only when EVERY axis
// of both maps is a power of two. K <= TN_SMALLK: the K offsets sit in LDS
// (k_einsum_smallk), past it they are decoded per k (k_einsum_anyk). The
// table decode (k_einsum_smallk_tbl) pays once ~4 offsets/thread are
// amortized over >= 8 elements and the per-element decode is actually deep;
// its index is 32-bit.
struct GatherChoice {
  int kernel;  // TN_GK_*
  int blocks;
  bool pow2;
};

inline GatherChoice plan_gather_kernel(const std::vector<AxisInfo>& oax,
                                       const std::vector<AxisInfo>& kax,
                                       u64 nout, u64 K) {
  GatherChoice c;
  c.pow2 = axes_pow2(oax) && axes_pow2(kax);
  c.blocks = grid_for(nout);
  if (K > TN_SMALLK) {
    c.kernel = c.pow2 ? TN_GK_ANYK_P2 : TN_GK_ANYK;
  } else if (c.pow2 && nout >= (1ull << 26) && nout < (1ull << 32) &&
             oax.size() >= 8) {
    c.kernel = TN_GK_SMALLK_TBL;
    if (c.blocks > 32768) c.blocks = 32768;
  } else {
    c.kernel = c.pow2 ? TN_GK_SMALLK_P2 : TN_GK_SMALLK;
  }
  return c;
}

// Tiled bit-permutation dot: both operands are contiguous pow2 spans of the
// same K elements in different axis orders. Fills *dp and returns the number
// of rest bits (one block per combination), or -1 when the form does not
// apply.
inline int plan_dot_tile(const Meta& A, const Meta& B, const AxisList& k_a,
                         const AxisList& k_b, DotPerm* dp) {
  struct BitSB {
    u64 sa, sb;
  };
  std::vector<BitSB> bits;
  for (int t = 0; t < k_a.n; ++t) {
    const u64 dim = A.dims[k_a[t]];
    const i64 sa = A.strides[k_a[t]], sb = B.strides[k_b[t]];
    if (dim == 1) continue;  // contributes no bits
    if ((dim & (dim - 1)) || sa <= 0 || sb <= 0) return -1;
    for (u64 d = 1; d < dim; d <<= 1)
      bits.push_back({(u64)sa * d, (u64)sb * d});
  }
  const int bb = TN_DOT_TILE_BBITS;
  const int nb = (int)bits.size();
  if (nb > TN_DOT_MAXBITS || nb <= TN_DOT_TILE_ABITS + bb) return -1;
  std::vector<int> byA(nb), byB(nb);
  for (int i = 0; i < nb; ++i) byA[i] = byB[i] = i;
  std::sort(byA.begin(), byA.end(),
            [&](int x, int y) { return bits[x].sa < bits[y].sa; });
  std::sort(byB.begin(), byB.end(),
            [&](int x, int y) { return bits[x].sb < bits[y].sb; });
  for (int i = 0; i < nb; ++i)
    if (bits[byA[i]].sa != (1ull << i) || bits[byB[i]].sb != (1ull << i))
      return -1;  // not a contiguous span on both sides
  std::vector<char> used(nb, 0);
  for (int i = 0; i < TN_DOT_TILE_ABITS; ++i) {
    used[byA[i]] = 1;
    dp->aB[i] = bits[byA[i]].sb;
  }
  int nbb = 0, nr = 0;
  for (int i = 0; i < nb && nbb < bb; ++i) {
    const int bi = byB[i];
    if (used[bi]) continue;
    dp->bA[nbb] = bits[bi].sa;
    dp->bB[nbb] = bits[bi].sb;
    used[bi] = 1;
    ++nbb;
  }
  for (int i = 0; i < nb; ++i) {
    if (used[byA[i]]) continue;
    dp->restA[nr] = bits[byA[i]].sa;
    dp->restB[nr] = bits[byA[i]].sb;
    ++nr;
  }
  dp->rbits = nr;
  return nr;
}

// Tiled bit-permutation copy (k_permute_tile): the axis list (outer..inner,
// dim and source stride; the destination is contiguous row-major over it)
// describes a pow2 bit permutation of >= 2^20 elements whose lowest source
// strides are coalescible. Fills *pp and returns the number of rest bits (one
// block per combination), or -1: the permute then runs through the gather
// permute k_permute_ct (strided views, non-pow2, tiny sizes).
inline int plan_permute_tile(const std::vector<AxisInfo>& ax, u64 elems,
                             PermPerm* pp) {
  if (elems < (1ull << 20) || elems > (1ull << TN_PERM_MAXBITS)) return -1;
  struct BitSD {
    u64 ss, sd;
  };
  std::vector<BitSD> bits;
  u64 dstride = 1;
  for (int i = (int)ax.size() - 1; i >= 0; --i) {
    const AxisInfo& a = ax[i];
    if (a.dim == 1) continue;  // contributes no bits; stride irrelevant
    if ((a.dim & (a.dim - 1)) || a.sa <= 0) return -1;
    for (u64 d = 1; d < a.dim; d <<= 1)
      bits.push_back({(u64)a.sa * d, dstride * d});
    dstride *= a.dim;
  }
  const int nb = (int)bits.size();
  if (nb <= TN_PERM_AB + TN_PERM_BB || (1ull << nb) != elems) return -1;
  std::vector<int> byS(nb), byD(nb);
  for (int i = 0; i < nb; ++i) byS[i] = byD[i] = i;
  std::sort(byS.begin(), byS.end(),
            [&](int x, int y) { return bits[x].ss < bits[y].ss; });
  std::sort(byD.begin(), byD.end(),
            [&](int x, int y) { return bits[x].sd < bits[y].sd; });
  // the a-bits (lane index) must be the TN_PERM_AB lowest SOURCE strides,
  // exactly 1..2^(AB-1), for coalesced reads. All other bits may carry
  // ARBITRARY source strides (the kernel sums per-bit offsets), which
  // admits sub-box permutes — e.g. the pack pipeline's K-windows, whose
  // fixed leading legs leave gaps in the source span. The destination
  // side is a full span by construction (suffix products above).
  for (int i = 0; i < TN_PERM_AB; ++i)
    if (bits[byS[i]].ss != (1ull << i)) return -1;
  std::vector<char> used(nb, 0);
  for (int i = 0; i < TN_PERM_AB; ++i) {
    used[byS[i]] = 1;
    pp->aD[i] = bits[byS[i]].sd;
  }
  int nbb = 0, nr = 0;
  for (int i = 0; i < nb && nbb < TN_PERM_BB; ++i) {
    const int bi = byD[i];
    if (used[bi]) continue;
    pp->bS[nbb] = bits[bi].ss;
    pp->bD[nbb] = bits[bi].sd;
    used[bi] = 1;
    ++nbb;
  }
  for (int i = 0; i < nb; ++i) {
    if (used[byS[i]]) continue;
    pp->restS[nr] = bits[byS[i]].ss;
    pp->restD[nr] = bits[byS[i]].sd;
    ++nr;
  }
  pp->rbits = nr;
  return nr;
}

// Which permute kernel launch_permute runs for this axis list
// (tn_step_plan's perm_* fields): 2 k_permute_tile, 1 k_permute_ct.
inline int permute_kind(const std::vector<AxisInfo>& ax, u64 elems) {
  PermPerm pp;
  return plan_permute_tile(ax, elems, &pp) >= 0 ? 2 : 1;
}

// The axis lists of a TTGT step's permutes. plan_step (the perm_* fields)
// and the executor (the launches) both build them here, so the plan and the
// launch cannot disagree.
// Pack of an operand into its GEMM layout (axes = a_axes / b_axes):
inline std::vector<AxisInfo> pack_axis_info(const Meta& t,
                                            const AxisList& axes) {
  std::vector<AxisInfo> ax;
  for (int axis : axes) ax.push_back({t.dims[axis], t.strides[axis], 0});
  return ax;
}

// Out permute: temporary C = [M legs (out order)][N legs (out order)] -> out
// order; the source stride of each out axis is its stride inside C.
inline std::vector<AxisInfo> out_axis_info(const StepPlan& p,
                                           const u64* out_shape, int out_nd) {
  std::vector<i64> tmp_stride(out_nd, 0);
  i64 stride = 1;
  for (int t = p.n_out.n - 1; t >= 0; --t) {
    tmp_stride[p.n_out[t]] = stride;
    stride *= (i64)out_shape[p.n_out[t]];
  }
  for (int t = p.m_out.n - 1; t >= 0; --t) {
    tmp_stride[p.m_out[t]] = stride;
    stride *= (i64)out_shape[p.m_out[t]];
  }
  std::vector<AxisInfo> ax;
  for (int i = 0; i < out_nd; ++i)
    ax.push_back({out_shape[i], tmp_stride[i], 0});
  return ax;
}

// K-window packs of a pipelined step: the operand's GEMM layout without the
// first npre K legs (those select the window).
inline std::vector<AxisInfo> window_a_axis_info(const StepPlan& p,
                                                const Meta& A, int npre) {
  std::vector<AxisInfo> ax;
  for (int o : p.m_out)
    ax.push_back({A.dims[p.apos[o]], A.strides[p.apos[o]], 0});
  for (int x = npre; x < p.k_a.n; ++x)
    ax.push_back({A.dims[p.k_a[x]], A.strides[p.k_a[x]], 0});
  return ax;
}

inline std::vector<AxisInfo> window_b_axis_info(const StepPlan& p,
                                                const Meta& B, int npre) {
  std::vector<AxisInfo> ax;
  for (int x = npre; x < p.k_b.n; ++x)
    ax.push_back({B.dims[p.k_b[x]], B.strides[p.k_b[x]], 0});
  for (int o : p.n_out)
    ax.push_back({B.dims[p.bpos[o]], B.strides[p.bpos[o]], 0});
  return ax;
}

// Build the bit-scatter map of a packed [row][k] (or [k][col]) layout:
// packed-index bit b -> source stride. Axes are outer..inner; the inner
// axis supplies the low bits. Fails on non-pow2 dims or non-positive
// strides (the step then takes the pack path).
inline bool build_ggmap(const Meta& t, const int* axes_r, int nr,
                        const int* axes_k, int nk, GatherGemmMap* m) {
  auto fill = [&](const int* axes, int count, u64* stride, int* nbits) {
    int nb = 0;
    for (int x = count - 1; x >= 0; --x) {
      u64 d = t.dims[axes[x]];
      if (d & (d - 1)) return false;
      if (d > 1 && t.strides[axes[x]] <= 0) return false;
      for (u64 v = 1; v < d; v <<= 1) {
        if (nb >= 34) return false;
        stride[nb++] = (u64)t.strides[axes[x]] * v;
      }
    }
    *nbits = nb;
    return true;
  };
  return fill(axes_r, nr, m->rstride, &m->rbits) &&
         fill(axes_k, nk, m->kstride, &m->kbits);
}

// Destination strides of the GEMM's row and column bits when C = [M legs in
// out order][N legs in out order] is stored straight into `out` (row-major
// in out order). Returns the run length r: the number of lowest destination
// bits that are, in order, the lowest column bits (2^r consecutive columns
// land contiguously), or -1 when a dim is no power of two or the bits do not
// fit the map.
inline int build_scatter_map(const u64* out_shape, int out_nd,
                             const AxisList& m_out, const AxisList& n_out,
                             ScatterMap* sm) {
  u64 ostride[TN_MAXR];
  u64 stride = 1;
  for (int i = out_nd - 1; i >= 0; --i) {
    if (out_shape[i] & (out_shape[i] - 1)) return -1;
    ostride[i] = stride;
    stride *= out_shape[i];
  }
  auto fill = [&](const AxisList& axes, u64* dst, int* nbits) {
    int nb = 0;
    for (int t = axes.n - 1; t >= 0; --t)
      for (u64 v = 1; v < out_shape[axes[t]]; v <<= 1) {
        if (nb >= 34) return false;
        dst[nb++] = ostride[axes[t]] * v;
      }
    *nbits = nb;
    return true;
  };
  if (!fill(m_out, sm->rstride, &sm->rbits) ||
      !fill(n_out, sm->cstride, &sm->cbits))
    return -1;
  int r = 0;
  while (r < sm->cbits && sm->cstride[r] == (1ull << r)) ++r;
  return r;
}

// Structural preconditions of k_zgemm_c128_glds_3m beyond purity: its
// staging offsets are 32-bit.
inline bool gemm3m_fits(u64 N, u64 K) {
  return (u64)MF_T * K * 16 <= 0xffffffffull &&
         (u64)MF_K * N * 16 <= 0xffffffffull;
}

// Profitability gate on (K, tile count), from the interleaved harness table
// (profiles/r03_kernel_stats.md): 3M beat the 4M kernel by 1.16-1.27x on
// every measured pure shape, K = 32..32768 and 256..131072 tiles. Nothing
// smaller was measured, so nothing smaller is admitted.
inline bool gemm3m_profitable(u64 K, u64 tiles) {
  return K >= 32 && tiles >= 256;
}

// Pack-pipeline choice: chunk the pack over P K-windows (the first npre K
// legs of A, kc = K / P each) so each window's permute overlaps the previous
// window's GEMM. The window GEMMs write split-K-style slices reduced at the
// end; the pack permutes (HBM-bound, ~4 TB/s) ride in the MFMA-bound GEMM's
// spare bandwidth (slice traffic streams at ~6 TB/s). Chosen when the model
// predicts a net win over the serial pack (the slice buffers cost (2p)·M·N
// extra traffic). Requires a packed A (a ready A's K-windows are strided); B
// may be packed or ready (row windows are contiguous).
inline void plan_pipeline(StepPlan& p, const Meta& A, u64 esize) {
  const u64 M = p.m, N = p.n, K = p.k;
  u64 packbytes = ((p.pack_a ? M * K : 0) + (p.pack_b ? K * N : 0)) * esize;
  struct Win {
    int p = 0, npre = 0;
    u64 kc = 0;
  } best, feas;  // best by the model; last (= finest) feasible
  double best_save = 0.0;
  u64 w = 1;
  u64 tiles_w = (M / MF_T) * ((N + MF_TN - 1) / MF_TN);
  for (int x = 0; x < p.k_a.n && w < 16; ++x) {
    w *= A.dims[p.k_a[x]];
    if (w < 2 || w > 16) continue;
    u64 kc = K / w;
    if (kc % MF_K || tiles_w < 256) continue;
    double save = 2.0 * (double)packbytes / 4e12 * (1.0 - 1.0 / w) -
                  2.0 * w * (double)(M * N * esize) / 6e12;
    feas = {(int)w, x + 1, kc};
    if (save > best_save) {
      best_save = save;
      best = feas;
    }
  }
  // measured gate (r02 A/B on hardware): marginal steps LOSE to the
  // serial pack (window-launch overhead + slice-reduce traffic), so
  // pipeline only when the predicted win is substantial and the pack
  // dwarfs the output (rqc36's 4-10x-ratio steps regressed ~12 ms;
  // syc49's 64x step gains ~12 ms)
  if (env_switch(ENV_PIPELINE_FORCE) && feas.p)
    best = feas;
  else if (best_save <= 5e-3 ||
           (double)packbytes < 8.0 * (double)(M * N * esize))
    best.p = 0;
  p.pipe_p = best.p;
  p.pipe_kc = best.p ? best.kc : 0;
  p.pipe_npre = best.p ? best.npre : 0;
}

// Plan one einsum step out = A · B (out contiguous row-major in out order).
// Returns TN_OK, or TN_ERR_INVALID with the message in *err.
inline int plan_step(bool c128, const u64* out_labels, const u64* out_shape,
                     int out_nd, const Meta& A, const Meta& B,
                     bool has_stream2, StepPlan* plan, std::string* err) {
  StepPlan& p = *plan;
  p = StepPlan();
  const u64 esize = c128 ? 16 : 8;
  auto fail = [&](const char* fmt, u64 v) {
    char buf[128];
    snprintf(buf, sizeof buf, fmt, (unsigned long long)v);
    *err = buf;
    return (int)TN_ERR_INVALID;
  };
  if (A.nd > TN_MAXR || B.nd > TN_MAXR || out_nd > TN_MAXR)
    return fail("tensor rank exceeds %llu", TN_MAXR);
  auto find = [](const Meta& t, u64 lab) {
    for (int i = 0; i < t.nd; ++i)
      if (t.labels[i] == lab) return i;
    return -1;
  };
  int* apos = p.apos;
  int* bpos = p.bpos;
  u64 M = 1, N = 1, K = 1;
  for (int i = 0; i < out_nd; ++i) {
    apos[i] = find(A, out_labels[i]);
    bpos[i] = find(B, out_labels[i]);
    if (apos[i] >= 0 && bpos[i] >= 0)
      return fail("out label %llu present in both inputs", out_labels[i]);
    if (apos[i] >= 0) {
      if (A.dims[apos[i]] != out_shape[i])
        return fail("dim mismatch on out label %llu", out_labels[i]);
      M *= out_shape[i];
      p.m_out.push_back(i);
    } else if (bpos[i] >= 0) {
      if (B.dims[bpos[i]] != out_shape[i])
        return fail("dim mismatch on out label %llu", out_labels[i]);
      N *= out_shape[i];
      p.n_out.push_back(i);
    } else {
      return fail("out label %llu not found in inputs", out_labels[i]);
    }
  }
  for (int i = 0; i < A.nd; ++i) {
    int j = find(B, A.labels[i]);
    if (j >= 0) {
      for (int o = 0; o < out_nd; ++o)
        if (out_labels[o] == A.labels[i])
          return fail("contracted label %llu appears in out", A.labels[i]);
      if (A.dims[i] != B.dims[j])
        return fail("K dim mismatch on label %llu", A.labels[i]);
      K *= A.dims[i];
      p.k_a.push_back(i);
      p.k_b.push_back(j);
    }
  }
  // every input label must be contracted (shared) or appear in out — traces
  // and repeated labels are outside the tensor_mult boundary contract
  // (contraction.rs:88-116 always passes the symmetric difference)
  auto in_out = [&](u64 lab) {
    for (int o = 0; o < out_nd; ++o)
      if (out_labels[o] == lab) return true;
    return false;
  };
  for (int i = 0; i < A.nd; ++i)
    if (find(B, A.labels[i]) < 0 && !in_out(A.labels[i]))
      return fail("label %llu of A neither contracted nor in out",
                  A.labels[i]);
  for (int i = 0; i < B.nd; ++i)
    if (find(A, B.labels[i]) < 0 && !in_out(B.labels[i]))
      return fail("label %llu of B neither contracted nor in out",
                  B.labels[i]);
  p.m = M;
  p.n = N;
  p.k = K;
  const u64 nout = M * N;

  // is each operand already contiguous in its GEMM layout? (reported for
  // every route; only the TTGT route acts on it)
  for (int o : p.m_out) p.a_axes.push_back(apos[o]);
  for (int i : p.k_a) p.a_axes.push_back(i);
  for (int j : p.k_b) p.b_axes.push_back(j);
  for (int o : p.n_out) p.b_axes.push_back(bpos[o]);
  auto is_ready = [](const Meta& t, const AxisList& axes) {
    if (axes.n != t.nd) return false;
    i64 stride = 1;
    for (int i = axes.n - 1; i >= 0; --i) {
      if (t.strides[axes[i]] != stride) return false;
      stride *= (i64)t.dims[axes[i]];
    }
    return true;
  };
  p.pack_a = !is_ready(A, p.a_axes);
  p.pack_b = !is_ready(B, p.b_axes);
  // does the GEMM's C = [M..][N..] equal `out` directly? True iff the M
  // legs all precede the N legs there (always so for the executor's
  // symmetric-difference order)
  p.direct = !(!p.m_out.empty() && !p.n_out.empty() &&
               p.m_out.back() > p.n_out.front());

  // ---- dot: scalar output, large K ----
  if (M == 1 && N == 1 && K > TN_SMALLK) {
    p.route = TN_ROUTE_DOT;
    // linear iff each axis' source stride equals its packed suffix product
    bool linear = true;
    i64 pstride = 1;
    for (int t = p.k_a.n - 1; t >= 0; --t) {
      if (A.strides[p.k_a[t]] != pstride || B.strides[p.k_b[t]] != pstride)
        linear = false;
      pstride *= (i64)A.dims[p.k_a[t]];
    }
    int tbits = -1;
    if (!linear && K >= (1ull << 20))
      tbits = plan_dot_tile(A, B, p.k_a, p.k_b, &p.dp);
    if (tbits > 0) {
      p.dot_form = TN_DOT_TILED;
      p.kind = 6;
      p.tbits = tbits;
      p.dot_blocks = 1ull << tbits;
    } else {
      p.dot_form = linear ? TN_DOT_LINEAR : TN_DOT_GATHER;
      p.kind = linear ? 5 : 1;  // 5 = linear (streaming) dot
      p.dot_blocks = (u64)std::min(grid_for(K), 2048);
    }
    p.ws_dot = p.dot_blocks * 16;  // double2 partials for either dtype
    return TN_OK;
  }

  // ---- smallk / anyk: small K, or skinny GEMM shapes ----
  // mid-K big shapes (e.g. M=2^20 N=2^10 K=32) run ~3x faster as a packed
  // MFMA GEMM than as an address-gather stream
  const bool skinny = (M < 16 || N < 16);
  const bool gemm_worthy = (K >= 16 && M >= MF_T && N >= MF_TN);
  p.gather_ok = (K <= TN_SMALLK || skinny);
  if (p.gather_ok) {
    // the kernel run_gather would launch: this step's own on the gather
    // route, the out-of-memory fallback's on the TTGT route
    const GatherChoice gc = plan_gather_kernel(
        gather_out_axis_info(p, out_shape, out_nd, A, B),
        gather_k_axis_info(p, A, B), nout, K);
    p.gather_kernel = gc.kernel;
    p.gather_blocks = gc.blocks;
  }
  if (p.gather_ok && !gemm_worthy) {
    p.route = TN_ROUTE_GATHER;
    p.kind = 0;
    return TN_OK;
  }

  // ---- TTGT: pack (if needed) + GEMM + unpack (if needed) ----
  p.route = TN_ROUTE_TTGT;
  p.kind = p.direct ? 2 : 3;
  const bool mfma_shape = (M >= 32 && N >= 32);
  const bool pure_shape =
      (M % MF_T == 0) && (N % MF_TN == 0) && (K % MF_K == 0);
  // gather-staged GEMM (c128): fold the pack permutes into the GEMM's LDS
  // staging when the shape is pure and every dim is pow2 — no pack
  // kernels, no pack workspace, no pack HBM traffic
  if (c128 && (p.pack_a || p.pack_b) && mfma_shape && pure_shape &&
      env_switch(ENV_GATHER_GEMM))
    p.gather_gemm =  // a_axes = [M.., K..], b_axes = [K.., N..]
        build_ggmap(A, p.a_axes.v, p.m_out.n, p.k_a.v, p.k_a.n, &p.gmA) &&
        build_ggmap(B, p.b_axes.v + p.k_b.n, p.n_out.n, p.k_b.v, p.k_b.n,
                    &p.gmB);
  if (has_stream2 && p.pack_a && mfma_shape && pure_shape &&
      !env_switch(ENV_NO_PIPELINE))
    plan_pipeline(p, A, esize);

  // the GEMM of the serial path (also what a pipelined step runs when its
  // window buffers cannot be had)
  const u64 row_tile_h = mfma_shape ? MF_T : GT;
  p.row_tiles = (M + row_tile_h - 1) / row_tile_h;
  p.col_tiles = (N + GT - 1) / GT;
  const u64 tiles = p.row_tiles * p.col_tiles;
  // split-K: with few tiles and deep K, slice K across extra blocks into
  // partial buffers + a reduce pass (fills the 256 CUs; a 64-tile K=2^20
  // GEMM goes from ~6 to ~50 TFLOP/s)
  u64 splitk = 1;
  if (tiles < 192 && K >= 256) {
    while (tiles * splitk < 256 && K / (splitk * 2) >= 64) splitk *= 2;
    if (splitk > 64) splitk = 64;
  }
  u64 kchunk = (K + splitk - 1) / splitk;
  kchunk = ((kchunk + MF_K - 1) / MF_K) * MF_K;  // tile-aligned
  p.kchunk = kchunk;
  p.splitk = (K + kchunk - 1) / kchunk;
  // The kernel does not depend on whether the split buffer is obtained:
  // the gated 3M route needs >= 256 tiles and split-K fewer than 192, and
  // the forced one ignores splitk.
  const bool pure = pure_shape && (kchunk % MF_K == 0);
  if (!mfma_shape) {
    p.kernel = TN_GEMM_V1;
  } else if (!c128) {
    p.kernel = pure ? TN_GEMM_C64_PURE : TN_GEMM_MFMA;
  } else if (p.gather_gemm) {
    // gather_gemm implies pure: its precondition covers M/N/K tiling and
    // kchunk is MF_K-rounded above
    p.kernel = TN_GEMM_C128_GATHER;
  } else {
    // 3M routing: pure, unsplit and past the profitability gate; "force"
    // drops the gate and the unsplit condition
    const int m3 = env_switch(ENV_GEMM3M);
    const bool use_3m =
        pure && m3 != GEMM3M_OFF && gemm3m_fits(N, K) &&
        (m3 == GEMM3M_FORCE ||
         (p.splitk == 1 && gemm3m_profitable(K, tiles)));
    p.kernel = use_3m ? TN_GEMM_C128_3M
                      : pure ? TN_GEMM_C128_PURE : TN_GEMM_C128_GLDS;
    p.gemm_pipe = use_3m && env_switch(ENV_GEMM3M_PIPE);
  }

  // scatter epilogue: a non-direct out order is written by the 3M GEMM
  // itself, no temporary C and no unpack permute. The run-length gate
  // (TN_SCATTER_MINRUN low column bits in place = 128 contiguous bytes per 8
  // columns) is the smallest store run the GEMM's epilogue is known to
  // sustain at full rate.
  if (!p.direct && c128 && p.kernel == TN_GEMM_C128_3M && p.splitk == 1 &&
      !p.pipe_p && !p.gather_gemm && env_switch(ENV_EPI_SCATTER) &&
      build_scatter_map(out_shape, out_nd, p.m_out, p.n_out, &p.smap) >=
          TN_SCATTER_MINRUN) {
    p.scatter_out = 1;
    p.kind = 2;  // no out permute runs
  }

  // workspace the step will ask for (a pipelined step's pack buffers hold
  // all P windows back to back)
  const bool packs = p.pipe_p || !p.gather_gemm;
  p.ws_tmp_c = (p.direct || p.scatter_out) ? 0 : nout * esize;
  p.ws_pack_a = (packs && p.pack_a) ? M * K * esize : 0;
  p.ws_pack_b = (packs && p.pack_b) ? K * N * esize : 0;
  p.ws_slices = (u64)p.pipe_p * nout * esize;
  p.ws_split = (!p.pipe_p && p.splitk > 1) ? p.splitk * nout * esize : 0;

  // which permute kernel each pack / unpack launches
  if (!p.gather_gemm && p.pack_a)
    p.perm_a = permute_kind(pack_axis_info(A, p.a_axes), M * K);
  if (!p.gather_gemm && p.pack_b)
    p.perm_b = permute_kind(pack_axis_info(B, p.b_axes), K * N);
  if (!p.direct && !p.scatter_out)
    p.perm_out = permute_kind(out_axis_info(p, out_shape, out_nd), nout);
  if (p.pipe_p) {
    p.pipe_perm_a = permute_kind(window_a_axis_info(p, A, p.pipe_npre),
                                 M * p.pipe_kc);
    if (p.pack_b)
      p.pipe_perm_b = permute_kind(window_b_axis_info(p, B, p.pipe_npre),
                                   p.pipe_kc * N);
  }
  return TN_OK;
}

// ---- walk plan ------------------------------------------------------------
// Everything about a whole flat replace-left path that follows from the path
// alone: the order each step stores its output in, and which operands of
// each step are packed one step early (the look-ahead pack).
//
// Stored orders. Today's rule is the symmetric difference of the operands'
// stored orders. When the next step c = s+1 reads step s's output as its A
// operand and would have to pack it inline (the one operand the look-ahead
// cannot hide: it does not exist while step s-1 runs), step s stores
//   [M' legs][K' legs]      M' = legs c keeps, K' = legs c contracts
// instead, provided plan_step admits that order to the scatter epilogue.
// Inside the K' group legs that come from M_s go first and legs from N_s
// last, so the N_s legs of K' are both the lowest column bits of step s's
// GEMM and the lowest destination bits: the run length the gate asks for.
// The M' group is free as far as step s goes; it takes the order step c
// wants its own rows in, so that c finds the operand ready whatever c's
// own stored order turns out to be. That makes the proposals depend on later
// steps only: one backward sweep over label sets proposes, one forward sweep
// over the stored orders decides (gate on the real operands, would-pack test
// on c, and no proposal that makes step s pack more inline than c saves).
// An output read as a B operand is left alone: its K' order is dictated by
// the other operand. The last step stores today's order, so results keep
// their legs. Slot labels always are the stored order.
//
// Look-ahead packs. While step s-1's GEMM runs (MFMA-bound, <10% of the HBM
// bandwidth a permute needs) the walk may pack step s's GEMM operands on a
// second stream, so that step s finds them ready. The rule, stated here
// once: step s is TTGT and not gather_gemm, and an operand is packed early
// iff the step's plan packs it and step s-1 did not produce it (it does not
// exist yet while s-1 runs). A prepacked slot is consumed by the very next
// step, so the orders this sweep sees are the orders the walk finds: the
// decision is a function of the path. Whether the walk acts on it (switch,
// arena, second stream, the allocations succeeding) is decided at run time;
// dispatch plans from the operands as they then sit on the device.

struct LayoutTensor {
  std::vector<u64> labels, dims;
};

// operands of one step that are packed while the previous step runs
struct EarlyPack {
  bool a = false, b = false;
  std::vector<int> a_axes, b_axes;  // axis orders of the packed layouts
  u64 a_elems = 0, b_elems = 0;     // m*k, k*n
};

struct LayoutPlan {
  bool valid = false;  // false: no plan, `err` says why; the walk refuses
  std::string err;
  std::vector<LayoutTensor> out;  // stored order of every step's output
  std::vector<int32_t> scatter_out;
  std::vector<EarlyPack> early;   // look-ahead pack of every step
  std::vector<u64> inline_pack_bytes;  // what the step packs, minus `early`
};

inline bool layout_has(const LayoutTensor& t, u64 lab) {
  for (u64 l : t.labels)
    if (l == lab) return true;
  return false;
}

// A-only legs in A order, then B-only legs in B order
inline void layout_symdiff(const LayoutTensor& a, const LayoutTensor& b,
                           LayoutTensor* out) {
  out->labels.clear();
  out->dims.clear();
  for (size_t x = 0; x < a.labels.size(); ++x)
    if (!layout_has(b, a.labels[x])) {
      out->labels.push_back(a.labels[x]);
      out->dims.push_back(a.dims[x]);
    }
  for (size_t x = 0; x < b.labels.size(); ++x)
    if (!layout_has(a, b.labels[x])) {
      out->labels.push_back(b.labels[x]);
      out->dims.push_back(b.dims[x]);
    }
}

// Meta of a contiguous row-major tensor with these labels and dims
inline void layout_meta(const LayoutTensor& t, Meta* m,
                        const void* data = nullptr) {
  m->nd = (int)t.labels.size();
  i64 stride = 1;
  for (int x = m->nd - 1; x >= 0; --x) {
    m->labels[x] = t.labels[x];
    m->dims[x] = t.dims[x];
    m->strides[x] = stride;
    stride *= (i64)t.dims[x];
  }
  m->data = data;
}

inline bool layout_plan_step(bool c128, const LayoutTensor& out,
                             const LayoutTensor& a, const LayoutTensor& b,
                             bool has_stream2, StepPlan* p,
                             std::string* err = nullptr) {
  Meta ma, mb;
  std::string local;
  layout_meta(a, &ma);
  layout_meta(b, &mb);
  return plan_step(c128, out.labels.data(), out.dims.data(),
                   (int)out.labels.size(), ma, mb, has_stream2, p,
                   err ? err : &local) == TN_OK;
}

inline void plan_layouts(bool c128, const std::vector<LayoutTensor>& leaves,
                         const u64* pairs, size_t nsteps, LayoutPlan* lp) {
  *lp = LayoutPlan();
  const size_t n = leaves.size();
  const u64 esize = c128 ? 16 : 8;
  // canonical walk: today's orders. Supplies the label sets of every step
  // and which step consumes each output.
  std::vector<LayoutTensor> canon(leaves), can_a(nsteps), can_b(nsteps),
      can_out(nsteps);
  std::vector<char> alive(n, 1);
  std::vector<long> producer(n, -1), consumer(nsteps, -1);
  std::vector<char> cons_as_a(nsteps, 0);
  auto refuse = [&](const char* why) { lp->err = why; };
  const char* const rank_err = "tensor rank exceeds 40";
  static_assert(TN_MAXR == 40, "rank_err names TN_MAXR");
  for (const LayoutTensor& t : leaves)
    if (t.labels.size() > (size_t)TN_MAXR) return refuse(rank_err);
  for (size_t s = 0; s < nsteps; ++s) {
    const u64 i = pairs[2 * s], j = pairs[2 * s + 1];
    if (i >= n || j >= n || i == j || !alive[i] || !alive[j])
      return refuse("invalid contraction path step");
    can_a[s] = canon[i];
    can_b[s] = canon[j];
    layout_symdiff(canon[i], canon[j], &can_out[s]);
    if (can_out[s].labels.size() > (size_t)TN_MAXR) return refuse(rank_err);
    if (producer[i] >= 0) {
      consumer[producer[i]] = (long)s;
      cons_as_a[producer[i]] = 1;
    }
    if (producer[j] >= 0) consumer[producer[j]] = (long)s;
    canon[i] = can_out[s];
    producer[i] = (long)s;
    alive[j] = 0;
  }

  // backward sweep: proposals
  std::vector<LayoutTensor> want(nsteps);
  const bool enabled = c128 && env_switch(ENV_EPI_SCATTER);
  for (size_t s = nsteps; enabled && s-- > 0;) {
    const long c = consumer[s];
    if (c != (long)s + 1 || !cons_as_a[s]) continue;
    const LayoutTensor& other = can_b[c];
    // the order step c wants its rows (= M' legs) in
    const LayoutTensor& row_src = want[c].labels.empty() ? can_out[s] : want[c];
    LayoutTensor d;
    for (size_t x = 0; x < row_src.labels.size(); ++x)
      if (layout_has(can_out[s], row_src.labels[x]) &&
          !layout_has(other, row_src.labels[x])) {
        d.labels.push_back(row_src.labels[x]);
        d.dims.push_back(row_src.dims[x]);
      }
    const size_t nrows = d.labels.size();
    for (size_t x = 0; x < can_out[s].labels.size(); ++x)
      if (layout_has(other, can_out[s].labels[x])) {
        d.labels.push_back(can_out[s].labels[x]);
        d.dims.push_back(can_out[s].dims[x]);
      }
    if (nrows == 0 || nrows == d.labels.size()) continue;
    StepPlan p;
    if (layout_plan_step(c128, d, can_a[s], can_b[s], false, &p) &&
        p.scatter_out)
      want[s] = d;
  }

  // forward sweep: decisions, on the stored orders
  std::vector<LayoutTensor> stored(leaves);
  lp->out.resize(nsteps);
  lp->scatter_out.assign(nsteps, 0);
  lp->early.assign(nsteps, EarlyPack());
  lp->inline_pack_bytes.assign(nsteps, 0);
  // the look-ahead pack of step s under plan p: the rule of the comment above
  auto early_of = [&](size_t s, const StepPlan& p) {
    EarlyPack e;
    if (s == 0 || p.route != TN_ROUTE_TTGT || p.gather_gemm) return e;
    const u64 made = pairs[2 * (s - 1)];  // slot step s-1 stored its output in
    e.a = p.pack_a && pairs[2 * s] != made;
    e.b = p.pack_b && pairs[2 * s + 1] != made;
    return e;
  };
  auto inline_bytes = [&](size_t s, const StepPlan& p) -> u64 {
    if (p.route != TN_ROUTE_TTGT || p.gather_gemm) return 0;
    const EarlyPack e = early_of(s, p);
    return ((p.pack_a && !e.a) ? p.m * p.k * esize : 0) +
           ((p.pack_b && !e.b) ? p.k * p.n * esize : 0);
  };
  for (size_t s = 0; s < nsteps; ++s) {
    const u64 i = pairs[2 * s], j = pairs[2 * s + 1];
    const LayoutTensor &A = stored[i], &B = stored[j];
    LayoutTensor base;
    layout_symdiff(A, B, &base);
    StepPlan pb;
    if (!layout_plan_step(c128, base, A, B, true, &pb, &lp->err)) return;
    LayoutTensor chosen = consumer[s] < 0 ? can_out[s] : base;
    StepPlan pc = pb;
    if (consumer[s] < 0 && chosen.labels != base.labels &&
        !layout_plan_step(c128, chosen, A, B, true, &pc, &lp->err))
      return;
    if (!want[s].labels.empty()) {
      // would step s+1 pack this output inline under today's order?
      const u64 oj = pairs[2 * (s + 1) + 1];
      LayoutTensor next_out;
      layout_symdiff(base, stored[oj], &next_out);
      StepPlan pn, pw;
      const bool packs_next =
          layout_plan_step(c128, next_out, base, stored[oj], true, &pn) &&
          pn.route == TN_ROUTE_TTGT && !pn.gather_gemm && pn.pack_a;
      if (packs_next && layout_plan_step(c128, want[s], A, B, true, &pw) &&
          pw.scatter_out &&
          inline_bytes(s, pw) < inline_bytes(s, pb) + pn.m * pn.k * esize) {
        chosen = want[s];
        pc = pw;
      }
    }
    EarlyPack& e = lp->early[s] = early_of(s, pc);
    if (e.a) e.a_axes.assign(pc.a_axes.begin(), pc.a_axes.end());
    if (e.b) e.b_axes.assign(pc.b_axes.begin(), pc.b_axes.end());
    e.a_elems = e.a ? pc.m * pc.k : 0;
    e.b_elems = e.b ? pc.k * pc.n : 0;
    lp->scatter_out[s] = pc.scatter_out;
    lp->inline_pack_bytes[s] = inline_bytes(s, pc);
    lp->out[s] = chosen;
    stored[i] = chosen;
  }
  lp->valid = true;
}

// ---- slice plan -----------------------------------------------------------
// Edge slicing contracts the network as a sum over the index values of some
// shared labels. Fixing a label's value removes that leg from the two leaves
// carrying it; the same path then contracts the reduced leaves. Everything
// that follows from (leaves, path, slice labels) is decided here, once:
//   - the reduced leaf set (sliced labels removed, order of the rest kept),
//     and the walk plan of the path over it: plan_layouts, unchanged, so the
//     sliced walk stores, packs and routes exactly as a fresh net holding
//     the reduced leaves would;
//   - per leaf and slice label, the element stride of that label in the
//     stored (full) leaf, 0 where the leaf does not carry it;
//   - the radices (dims of the slice labels) and the assignment count.
// Assignment t decodes with the FIRST label most significant (the order of
// itertools.product): digit x = (t / weight[x]) % radix[x], weight[x] the
// product of the radices after x. The source offset of a sliced leaf under
// assignment t is the sum over labels of digit * stride.

struct SlicePlan {
  bool valid = false;  // false: refused, `err` says why
  std::string err;
  std::vector<u64> labels, radices, weights;  // per slice label
  u64 count = 1;                              // number of assignments
  std::vector<LayoutTensor> reduced;          // per leaf
  std::vector<u64> strides;                   // nleaves x nslice, row-major
  std::vector<char> sliced;                   // per leaf: carries a label
  LayoutPlan layout;                          // plan_layouts over `reduced`
};

inline void plan_slices(bool c128, const std::vector<LayoutTensor>& leaves,
                        const u64* pairs, size_t nsteps,
                        const u64* slice_labels, size_t nlabels,
                        SlicePlan* sp) {
  *sp = SlicePlan();
  const size_t n = leaves.size();
  char buf[160];
  auto refuse = [&](const char* fmt, u64 a, u64 b = 0) {
    snprintf(buf, sizeof buf, fmt, (unsigned long long)a,
             (unsigned long long)b);
    sp->err = buf;
  };
  // the legs the path leaves open: a legs-only walk of the path
  std::vector<std::vector<u64>> legs(n);
  std::vector<char> alive(n, 1);
  for (size_t x = 0; x < n; ++x) legs[x] = leaves[x].labels;
  for (size_t s = 0; s < nsteps; ++s) {
    const u64 i = pairs[2 * s], j = pairs[2 * s + 1];
    if (i >= n || j >= n || i == j || !alive[i] || !alive[j]) {
      sp->err = "invalid contraction path step";
      return;
    }
    std::vector<u64> out;
    for (u64 l : legs[i])
      if (std::find(legs[j].begin(), legs[j].end(), l) == legs[j].end())
        out.push_back(l);
    for (u64 l : legs[j])
      if (std::find(legs[i].begin(), legs[i].end(), l) == legs[i].end())
        out.push_back(l);
    legs[i].swap(out);
    legs[j].clear();
    alive[j] = 0;
  }
  sp->labels.assign(slice_labels, slice_labels + nlabels);
  sp->radices.assign(nlabels, 0);
  sp->strides.assign(n * nlabels, 0);
  sp->sliced.assign(n, 0);
  for (size_t x = 0; x < nlabels; ++x) {
    const u64 lab = slice_labels[x];
    for (size_t y = 0; y < x; ++y)
      if (slice_labels[y] == lab)
        return refuse("slice label %llu is listed twice", lab);
    u64 carriers = 0;
    for (size_t t = 0; t < n; ++t) {
      const LayoutTensor& lt = leaves[t];
      u64 stride = 1;
      for (size_t a = lt.labels.size(); a-- > 0;) {
        if (lt.labels[a] == lab) {
          if (sp->strides[t * nlabels + x])
            return refuse("slice label %llu is repeated within leaf %llu", lab,
                          (u64)t);
          ++carriers;
          sp->radices[x] = lt.dims[a];
          sp->strides[t * nlabels + x] = stride;
          sp->sliced[t] = 1;
        }
        stride *= lt.dims[a];
      }
    }
    if (carriers == 0) return refuse("slice label %llu is in no leaf", lab);
    for (size_t t = 0; t < n; ++t)
      if (alive[t] && std::find(legs[t].begin(), legs[t].end(), lab) !=
                          legs[t].end())
        return refuse("slice label %llu is a leg of the final tensor", lab);
    if (carriers != 2)
      return refuse("slice label %llu is carried by %llu leaves, not two", lab,
                    carriers);
  }
  sp->weights.assign(nlabels, 1);
  for (size_t x = nlabels; x-- > 0;) {
    sp->weights[x] = sp->count;
    if (__builtin_mul_overflow(sp->count, sp->radices[x], &sp->count))
      return refuse("assignment count of %llu slice labels overflows 64 bits",
                    (u64)nlabels);
  }
  sp->reduced.resize(n);
  for (size_t t = 0; t < n; ++t)
    for (size_t a = 0; a < leaves[t].labels.size(); ++a)
      if (std::find(sp->labels.begin(), sp->labels.end(),
                    leaves[t].labels[a]) == sp->labels.end()) {
        sp->reduced[t].labels.push_back(leaves[t].labels[a]);
        sp->reduced[t].dims.push_back(leaves[t].dims[a]);
      }
  plan_layouts(c128, sp->reduced, pairs, nsteps, &sp->layout);
  if (!sp->layout.valid) {
    sp->err = sp->layout.err;
    return;
  }
  sp->valid = true;
}

// ---- batch labels ---------------------------------------------------------
// A step-batch label is carried by both operands and kept in out (not
// summed); the caller lists the labels that may act so. plan_step_batched
// splits those axes off, plans ONE batch element with plan_step (metas with
// the batch axes removed, strides kept) and classifies the step:
//   NONE    no step-batch label: the plan is plan_step's, field for field
//   GATHER  element on the gather route: one launch of the gather kernels
//           over all of out; a batch axis carries a stride in both operands
//   GEMM    element is an unsplit TTGT GEMM of fewer than TN_BATCH_MAXTILES
//           tiles: operands packed to [batch][M][K] / [batch][K][N] (one
//           permute each, none when already so), one k_zgemm_batched launch
//   LOOP    the rest (dot, split-K, an element that fills the device alone):
//           the element step, `batch` times, on offset views
// The step-batch labels lead out, so element b of out is the contiguous
// block at out + b*M*N, b the row-major index over the batch axes in out
// order.

// one workgroup per CU of the MI355X: an element with that many tiles gains
// nothing from sharing a launch
#define TN_BATCH_MAXTILES 256
#define BG_T 64  // k_zgemm_batched tile edge

struct BatchPlan : tn_batch_plan {
  StepPlan ep;                  // the element plan, with its axis lists
  int nb = 0;                   // step-batch axes = the first nb axes of out
  int ba[TN_MAXR], bb[TN_MAXR]; // their positions in A / B, in out order
  u64 bdim[TN_MAXR];
  Meta Ae, Be;                  // one element: batch axes removed
  int a_el[TN_MAXR], b_el[TN_MAXR];  // full-operand axis of each element axis
  // GEMM class
  u64 row_tiles = 0, col_tiles = 0;  // BG_T x BG_T tiles of one element
};

// source offset (elements) of batch element b in an operand
inline i64 batch_offset(const BatchPlan& p, const Meta& t, const int* pos,
                        u64 b) {
  i64 off = 0;
  for (int x = p.nb - 1; x >= 0; --x) {
    off += (i64)(b % p.bdim[x]) * t.strides[pos[x]];
    b /= p.bdim[x];
  }
  return off;
}

// Pack of a whole batched operand: [batch axes in out order][element axes in
// GEMM order]
inline std::vector<AxisInfo> batch_pack_axis_info(const BatchPlan& p,
                                                  const Meta& t,
                                                  const int* pos,
                                                  const Meta& te,
                                                  const AxisList& axes) {
  std::vector<AxisInfo> ax;
  for (int x = 0; x < p.nb; ++x)
    ax.push_back({t.dims[pos[x]], t.strides[pos[x]], 0});
  for (int axis : axes) ax.push_back({te.dims[axis], te.strides[axis], 0});
  return ax;
}

// Out permute of a batched GEMM: temporary [batch][M legs][N legs] -> out
inline std::vector<AxisInfo> batch_out_axis_info(const BatchPlan& p,
                                                 const u64* out_shape,
                                                 int out_nd) {
  std::vector<AxisInfo> ax(p.nb), el =
      out_axis_info(p.ep, out_shape + p.nb, out_nd - p.nb);
  i64 stride = (i64)p.ep.nout();
  for (int x = p.nb - 1; x >= 0; --x) {
    ax[x] = {p.bdim[x], stride, 0};
    stride *= (i64)p.bdim[x];
  }
  ax.insert(ax.end(), el.begin(), el.end());
  return ax;
}

// Batch axes of a GATHER-class launch, ahead of the element's out axes
inline std::vector<AxisInfo> batch_lead_axis_info(const BatchPlan& p,
                                                  const Meta& A,
                                                  const Meta& B) {
  std::vector<AxisInfo> lead;
  for (int x = 0; x < p.nb; ++x)
    lead.push_back({p.bdim[x], A.strides[p.ba[x]], B.strides[p.bb[x]]});
  return lead;
}

inline bool axis_info_ready(const std::vector<AxisInfo>& ax) {
  i64 stride = 1;
  for (int i = (int)ax.size() - 1; i >= 0; --i) {
    if (ax[i].sa != stride) return false;
    stride *= (i64)ax[i].dim;
  }
  return true;
}

inline int plan_step_batched(bool c128, const u64* out_labels,
                             const u64* out_shape, int out_nd, const Meta& A,
                             const Meta& B, const u64* batch_labels,
                             size_t nbatch, bool has_stream2, BatchPlan* plan,
                             std::string* err) {
  BatchPlan& p = *plan;
  p = BatchPlan();
  const u64 esize = c128 ? 16 : 8;
  auto fail = [&](const char* fmt, u64 v) {
    char buf[128];
    snprintf(buf, sizeof buf, fmt, (unsigned long long)v);
    *err = buf;
    return (int)TN_ERR_INVALID;
  };
  if (A.nd > TN_MAXR || B.nd > TN_MAXR || out_nd > TN_MAXR)
    return fail("tensor rank exceeds %llu", TN_MAXR);
  auto find = [](const Meta& t, u64 lab) {
    for (int i = 0; i < t.nd; ++i)
      if (t.labels[i] == lab) return i;
    return -1;
  };
  // the step-batch labels, by their position in out
  int at_out[TN_MAXR];  // out axis -> 1 when a step-batch label sits there
  for (int o = 0; o < out_nd; ++o) at_out[o] = 0;
  p.batch = 1;
  for (size_t x = 0; x < nbatch; ++x) {
    const u64 lab = batch_labels[x];
    bool seen = false;
    for (size_t y = 0; y < x; ++y) seen = seen || batch_labels[y] == lab;
    const int ia = find(A, lab), ib = find(B, lab);
    if (seen || ia < 0 || ib < 0) continue;  // free label, or not here
    int o = 0;
    while (o < out_nd && out_labels[o] != lab) ++o;
    if (o == out_nd) return fail("batch label %llu missing from out", lab);
    if (A.dims[ia] != B.dims[ib] || A.dims[ia] != out_shape[o])
      return fail("batch dim mismatch on label %llu", lab);
    at_out[o] = 1;
    ++p.nb;
  }
  for (int o = 0; o < p.nb; ++o) {
    if (!at_out[o]) {
      *err = "batch labels must lead out";
      return (int)TN_ERR_INVALID;
    }
    p.ba[o] = find(A, out_labels[o]);
    p.bb[o] = find(B, out_labels[o]);
    p.bdim[o] = out_shape[o];
    p.batch *= out_shape[o];
  }
  // one element: the operands without the step-batch axes, strides kept
  auto strip = [&](const Meta& t, const int* pos, Meta* e, int* el) {
    e->nd = 0;
    e->data = t.data;
    for (int i = 0; i < t.nd; ++i) {
      bool is_batch = false;
      for (int x = 0; x < p.nb; ++x) is_batch = is_batch || pos[x] == i;
      if (is_batch) continue;
      e->labels[e->nd] = t.labels[i];
      e->dims[e->nd] = t.dims[i];
      e->strides[e->nd] = t.strides[i];
      el[e->nd++] = i;
    }
  };
  strip(A, p.ba, &p.Ae, p.a_el);
  strip(B, p.bb, &p.Be, p.b_el);
  if (int rc = plan_step(c128, out_labels + p.nb, out_shape + p.nb,
                         out_nd - p.nb, p.Ae, p.Be, has_stream2, &p.ep, err))
    return rc;
  p.elem = p.ep;
  p.dispatches = 1;
  p.cls = TN_BATCH_NONE;
  if (p.nb == 0) return TN_OK;

  const StepPlan& e = p.ep;
  p.row_tiles = (e.m + BG_T - 1) / BG_T;
  p.col_tiles = (e.n + BG_T - 1) / BG_T;
  const u64 tiles = p.row_tiles * p.col_tiles;
  if (e.route == TN_ROUTE_GATHER) {
    p.cls = TN_BATCH_GATHER;
    // one launch over all of out: the batch axes lead the out map
    p.gather_kernel =
        plan_gather_kernel(
            gather_out_axis_info(e, out_shape + p.nb, out_nd - p.nb, p.Ae,
                                 p.Be, batch_lead_axis_info(p, A, B)),
            gather_k_axis_info(e, p.Ae, p.Be), p.batch * e.nout(), e.k)
            .kernel;
  } else if (e.route == TN_ROUTE_TTGT && e.splitk == 1 &&
             e.row_tiles * e.col_tiles < TN_BATCH_MAXTILES &&
             tiles < (1ull << 31) / p.batch &&  // the grid is 32-bit
             env_switch(ENV_BATCH_GEMM)) {
    p.cls = TN_BATCH_GEMM;
    if (!axis_info_ready(batch_pack_axis_info(p, A, p.ba, p.Ae, e.a_axes)))
      p.ws_pack_a = p.batch * e.m * e.k * esize;
    if (!axis_info_ready(batch_pack_axis_info(p, B, p.bb, p.Be, e.b_axes)))
      p.ws_pack_b = p.batch * e.k * e.n * esize;
  } else {
    p.cls = TN_BATCH_LOOP;
    p.dispatches = p.batch;
  }
  return TN_OK;
}

// workspace a batched step asks for beyond its output
inline u64 batch_step_ws(const BatchPlan& p, u64 esize) {
  const tn_step_plan& e = p.elem;
  const u64 elem_ws = e.ws_pack_a + e.ws_pack_b + e.ws_tmp_c + e.ws_slices +
                      e.ws_split + e.ws_dot;
  if (p.cls == TN_BATCH_GATHER) return 0;
  if (p.cls == TN_BATCH_GEMM)
    return p.ws_pack_a + p.ws_pack_b +
           (e.direct ? 0 : p.batch * e.m * e.n * esize);
  return elem_ws;  // NONE, LOOP: one element at a time
}

// The walk plan of a batched contraction: stored order and class of every
// step of a flat replace-left path. Order rule: [labels of L carried by both
// operands, in L's order][A-only legs in A order][B-only legs in B order];
// a label of L carried by one operand only counts as A-only / B-only. Every
// batched step then writes [batch][M legs][N legs] directly. No scatter
// epilogue, no look-ahead pack, no layout proposals.
struct BatchWalkPlan {
  bool valid = false;
  std::string err;
  std::vector<LayoutTensor> out;  // stored order of every step's output
  std::vector<int32_t> cls;
  std::vector<u64> ws_bytes;
};

inline void plan_batch_walk(bool c128, const std::vector<LayoutTensor>& leaves,
                            const u64* pairs, size_t nsteps,
                            const u64* batch_labels, size_t nbatch,
                            BatchWalkPlan* bw) {
  *bw = BatchWalkPlan();
  const size_t n = leaves.size();
  const u64 esize = c128 ? 16 : 8;
  char buf[160];
  auto refuse = [&](const char* fmt, u64 a) {
    snprintf(buf, sizeof buf, fmt, (unsigned long long)a);
    bw->err = buf;
  };
  for (size_t x = 0; x < nbatch; ++x) {
    const u64 lab = batch_labels[x];
    for (size_t y = 0; y < x; ++y)
      if (batch_labels[y] == lab)
        return refuse("batch label %llu is listed twice", lab);
    u64 dim = 0;
    for (const LayoutTensor& t : leaves)
      for (size_t a = 0; a < t.labels.size(); ++a) {
        if (t.labels[a] != lab) continue;
        if (dim && t.dims[a] != dim)
          return refuse("batch label %llu has differing dims across leaves",
                        lab);
        dim = t.dims[a];
      }
    if (!dim) return refuse("batch label %llu is in no leaf", lab);
  }
  for (const LayoutTensor& t : leaves)
    if (t.labels.size() > (size_t)TN_MAXR)
      return refuse("tensor rank exceeds %llu", TN_MAXR);
  std::vector<LayoutTensor> stored(leaves);
  std::vector<char> alive(n, 1);
  bw->out.resize(nsteps);
  bw->cls.assign(nsteps, TN_BATCH_NONE);
  bw->ws_bytes.assign(nsteps, 0);
  for (size_t s = 0; s < nsteps; ++s) {
    const u64 i = pairs[2 * s], j = pairs[2 * s + 1];
    if (i >= n || j >= n || i == j || !alive[i] || !alive[j]) {
      bw->err = "invalid contraction path step";
      return;
    }
    const LayoutTensor &A = stored[i], &B = stored[j];
    LayoutTensor o, rest;
    for (size_t x = 0; x < nbatch; ++x)
      for (size_t a = 0; a < A.labels.size(); ++a)
        if (A.labels[a] == batch_labels[x] && layout_has(B, batch_labels[x])) {
          o.labels.push_back(A.labels[a]);
          o.dims.push_back(A.dims[a]);
        }
    layout_symdiff(A, B, &rest);
    o.labels.insert(o.labels.end(), rest.labels.begin(), rest.labels.end());
    o.dims.insert(o.dims.end(), rest.dims.begin(), rest.dims.end());
    if (o.labels.size() > (size_t)TN_MAXR)
      return refuse("tensor rank exceeds %llu", TN_MAXR);
    Meta ma, mb;
    layout_meta(A, &ma);
    layout_meta(B, &mb);
    BatchPlan bp;
    if (plan_step_batched(c128, o.labels.data(), o.dims.data(),
                          (int)o.labels.size(), ma, mb, batch_labels, nbatch,
                          true, &bp, &bw->err) != TN_OK)
      return;
    bw->cls[s] = bp.cls;
    bw->ws_bytes[s] = batch_step_ws(bp, esize);
    bw->out[s] = o;
    stored[i] = o;
    alive[j] = 0;
  }
  bw->valid = true;
}

// ---- sampling the final tensor (tn_sample_*_dev, tn_net_sample) ------------
//
// p[i] = re^2 + im^2 in f64 (two products, one add, no fused multiply-add).
// S[j] is the sum of p over chunk j, C the inclusive prefix of S added one
// after another in ascending j, total = C[last]. A shot with uniform u draws
// t = u * total, the chunk sample_pick_chunk names, and in it the element
// sample_pick_in_chunk names for t - C[j-1]. The kernels restate the two pick
// functions; sample_plan_check runs them on the host.

#define TN_SAMPLE_CHUNK 4096   // elements per chunk: one block of pass 1
#define TN_SAMPLE_THREADS 256  // block size of all three kernels
#define TN_SAMPLE_SLAB 16      // consecutive elements one draw thread scans
#define TN_SAMPLE_SCAN_TILE 2048  // entries k_prob_scan holds in LDS per pass

static_assert(TN_SAMPLE_THREADS * TN_SAMPLE_SLAB == TN_SAMPLE_CHUNK,
              "one draw block covers one chunk");

struct SamplePlan {
  bool valid = false;
  std::string err;
  u64 chunk = TN_SAMPLE_CHUNK;
  u64 nchunks = 0;
  u64 grid_sums = 0;  // k_prob_chunk_sums: one block per chunk
  u64 grid_scan = 0;  // k_prob_scan: one block
  u64 grid_draw = 0;  // k_sample_draw: one block per shot; 0 = not launched
  // C[nchunks] | u[nshots] | idx[nshots] | total, in this order. The *_dev
  // entry points use the C part only (off_u bytes).
  u64 off_u = 0, off_idx = 0, off_total = 0, ws_bytes = 0;
};

inline void plan_sample(u64 n, u64 nshots, u64 esize, SamplePlan* sp) {
  *sp = SamplePlan();
  if (esize != 16 && esize != 8) {
    sp->err = "dtype must be 0 (c128) or 1 (c64)";
    return;
  }
  if (n == 0) {
    sp->err = "tensor has no elements";
    return;
  }
  if (n > ~(u64)0 / esize) {
    sp->err = "tensor size overflows 64 bits";
    return;
  }
  sp->nchunks = (n - 1) / TN_SAMPLE_CHUNK + 1;
  // a grid is at most 2^31 - 1 blocks
  if (sp->nchunks > 0x7fffffffull || nshots > 0x7fffffffull) {
    sp->err = "more chunks or shots than one grid holds";
    return;
  }
  sp->grid_sums = sp->nchunks;
  sp->grid_scan = 1;
  sp->grid_draw = nshots;
  sp->off_u = sp->nchunks * 8;
  sp->off_idx = sp->off_u + nshots * 8;
  sp->off_total = sp->off_idx + nshots * 8;
  sp->ws_bytes = sp->off_total + 8;
  sp->valid = true;
}

// The chunk of a shot: the first j with C[j] > t; where there is none
// (rounding of u * total at u next to 1) the last chunk that added mass, the
// last j with C[j] > C[j-1], C[-1] = 0. C is non-decreasing, so both are
// bisections: the last chunk that added mass is the first whose C reaches
// C[last]. 0 when no chunk added mass (total == 0, refused before any draw).
// A chunk whose S is positive but is lost in the rounding of C[j-1] + S[j]
// counts as having added none.
inline u64 sample_pick_chunk(const double* C, u64 nchunks, double t) {
  u64 lo = 0, hi = nchunks;  // C[x] <= t for x < lo, C[x] > t for x >= hi
  while (lo < hi) {
    const u64 mid = lo + (hi - lo) / 2;
    if (C[mid] > t)
      hi = mid;
    else
      lo = mid + 1;
  }
  if (lo < nchunks) return lo;
  const double top = C[nchunks - 1];
  lo = 0, hi = nchunks - 1;  // C[x] < top for x < lo, C[hi] reaches top
  while (lo < hi) {
    const u64 mid = lo + (hi - lo) / 2;
    if (C[mid] < top)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

// The element of a shot inside its chunk: the first i with p[i] > 0 and
// r > t, r the running sum in element order, taken slab by slab as
// k_sample_draw takes it:
// the sum of each slab of TN_SAMPLE_SLAB elements starts from zero, the slab
// sums in front of a slab are added one after another in ascending order, and
// the slab's own elements are added to that in order. Where the p are exactly
// representable sums this is the plain left-to-right sum, under which p > 0
// holds of itself at the first r > t; with slabs a slab's offset may round
// past t where no r in front of it did, and the test on p keeps an element
// without mass from being drawn there. Where no element qualifies, the last
// with p > 0; 0 for a chunk without mass, which sample_pick_chunk never
// names. NaN compares false everywhere and ends in the same clamp.
inline u64 sample_pick_in_chunk(const double* p, u64 len, double t) {
  double off = 0.0;
  for (u64 base = 0; base < len; base += TN_SAMPLE_SLAB) {
    const u64 end = std::min<u64>(base + TN_SAMPLE_SLAB, len);
    double r = off, slab = 0.0;
    for (u64 i = base; i < end; ++i) {
      r += p[i];
      if (p[i] > 0.0 && r > t) return i;
      slab += p[i];
    }
    off += slab;
  }
  for (u64 i = len; i-- > 0;)
    if (p[i] > 0.0) return i;
  return 0;
}

#endif  // TNC_STEP_PLAN_HPP
