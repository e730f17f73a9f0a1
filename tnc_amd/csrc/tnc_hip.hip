// tnc_hip — MI355X-native (gfx950/CDNA4) tensor-network contraction library.
//
// Implements the C ABI of include/tnc_hip.h: pairwise complex128 einsum
// (the tblis::tensor_mult replacement, reference call site
// tnc/src/tensornetwork/contraction.rs:111-113) as hand-written HIP kernels,
// and the device-resident replace-left network executor (the
// contract_tensor_network replacement, contraction.rs:35-68).
//
// Kernel classes (DESIGN.md "Data layout & kernels"):
//   smallk — K <= 64: one thread per output element, K-offsets precomputed
//            in LDS, gathered strided reads, coalesced writes. Covers gate
//            applications (K,N tiny, M huge) and outer products (K == 1).
//   anyk   — skinny shapes with K > 64: same, offsets computed inline.
//   dot    — M == N == 1, large K: two-pass block reduction.
//   zgemm  — TTGT: pack (index permute, skipped when the operand is already
//            contiguous in GEMM order) + tiled complex GEMM
//            (v_mfma_f64_16x16x4_f64 for large tiles, LDS-tiled VALU
//            fallback for ragged shapes) + optional unpack permute.
//
// All index maps have a pow2 fast path (every bond dim is 2 in the benchmark
// configs => index maps are pure bit shuffles) and a general div/mod path
// (the reference's golden-vector tensors use dims 3..8).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/tnc_hip.h"
#include "step_plan.hpp"

// ---------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------

static thread_local std::string g_last_error;

extern "C" const char* tn_last_error(void) { return g_last_error.c_str(); }

#define FAILV(code, ...)                       \
  do {                                         \
    char buf_[512];                            \
    snprintf(buf_, sizeof(buf_), __VA_ARGS__); \
    g_last_error = buf_;                       \
    return (code);                             \
  } while (0)

#define HIP_CHECK(expr)                                                 \
  do {                                                                  \
    hipError_t err_ = (expr);                                           \
    if (err_ != hipSuccess)                                             \
      FAILV(TN_ERR_HIP, "%s failed: %s (%s:%d)", #expr,                 \
            hipGetErrorString(err_), __FILE__, __LINE__);               \
  } while (0)

// ---------------------------------------------------------------------------
// gather maps (GatherMap, build_map: step_plan.hpp)
// ---------------------------------------------------------------------------

template <bool P2>
__device__ __forceinline__ void gather2(const GatherMap& m, u64 p, i64& oa,
                                        i64& ob) {
  i64 a = 0, b = 0;
  for (int i = 0; i < m.n; ++i) {
    u64 c = P2 ? ((p >> m.pstride[i]) & m.dim[i])
               : ((p / m.pstride[i]) % m.dim[i]);
    a += (i64)c * m.sa[i];
    b += (i64)c * m.sb[i];
  }
  oa = a;
  ob = b;
}

template <bool P2>
__device__ __forceinline__ i64 gather1(const GatherMap& m, u64 p) {
  i64 a = 0;
  for (int i = 0; i < m.n; ++i) {
    u64 c = P2 ? ((p >> m.pstride[i]) & m.dim[i])
               : ((p / m.pstride[i]) % m.dim[i]);
    a += (i64)c * m.sa[i];
  }
  return a;
}

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------

template <bool P2, typename CT>
__global__ void k_einsum_smallk(const CT* __restrict__ A,
                                const CT* __restrict__ B,
                                CT* __restrict__ C, u64 nout,
                                GatherMap omap, GatherMap kmap, int K) {
  using RT = decltype(CT{}.x);
  __shared__ i64 koffA[TN_SMALLK];
  __shared__ i64 koffB[TN_SMALLK];
  if (threadIdx.x < (unsigned)K) {
    i64 ka, kb;
    gather2<P2>(kmap, threadIdx.x, ka, kb);
    koffA[threadIdx.x] = ka;
    koffB[threadIdx.x] = kb;
  }
  __syncthreads();
  for (u64 p = blockIdx.x * (u64)blockDim.x + threadIdx.x; p < nout;
       p += gridDim.x * (u64)blockDim.x) {
    i64 oa, ob;
    gather2<P2>(omap, p, oa, ob);
    RT re = 0, im = 0;
    for (int k = 0; k < K; ++k) {
      CT a = A[oa + koffA[k]];
      CT b = B[ob + koffB[k]];
      re = fma(a.x, b.x, fma(-a.y, b.y, re));
      im = fma(a.x, b.y, fma(a.y, b.x, im));
    }
    C[p] = CT{re, im};
  }
}

// Table-decode smallk: for pow2 maps the source offset is additive over the
// index bits, so oa(p)/ob(p) collapse to four 8-bit LDS lookups instead of
// an n-axis shift/mask loop per element. The decode, not memory, bounds
// k_einsum_smallk on rank-~30 intermediates (measured 0.8 TB/s effective on
// a 2^30-element gate-apply step). Requires nout < 2^32.
template <typename CT>
__global__ void k_einsum_smallk_tbl(const CT* __restrict__ A,
                                    const CT* __restrict__ B,
                                    CT* __restrict__ C, u64 nout,
                                    GatherMap omap, GatherMap kmap, int K) {
  using RT = decltype(CT{}.x);
  __shared__ i64 ta[4][256], tb[4][256];
  __shared__ i64 koffA[TN_SMALLK];
  __shared__ i64 koffB[TN_SMALLK];
  for (int t = threadIdx.x; t < 1024; t += blockDim.x) {
    const int ti = t >> 8, e = t & 255;
    i64 oa, ob;
    gather2<true>(omap, (u64)e << (8 * ti), oa, ob);
    ta[ti][e] = oa;
    tb[ti][e] = ob;
  }
  if (threadIdx.x < (unsigned)K) {
    i64 ka, kb;
    gather2<true>(kmap, threadIdx.x, ka, kb);
    koffA[threadIdx.x] = ka;
    koffB[threadIdx.x] = kb;
  }
  __syncthreads();
  for (u64 p = blockIdx.x * (u64)blockDim.x + threadIdx.x; p < nout;
       p += gridDim.x * (u64)blockDim.x) {
    const unsigned lo = (unsigned)p;
    const i64 oa = ta[0][lo & 255] + ta[1][(lo >> 8) & 255] +
                   ta[2][(lo >> 16) & 255] + ta[3][lo >> 24];
    const i64 ob = tb[0][lo & 255] + tb[1][(lo >> 8) & 255] +
                   tb[2][(lo >> 16) & 255] + tb[3][lo >> 24];
    RT re = 0, im = 0;
    for (int k = 0; k < K; ++k) {
      CT a = A[oa + koffA[k]];
      CT b = B[ob + koffB[k]];
      re = fma(a.x, b.x, fma(-a.y, b.y, re));
      im = fma(a.x, b.y, fma(a.y, b.x, im));
    }
    C[p] = CT{re, im};
  }
}

// skinny shapes with K > TN_SMALLK: offsets computed inline per k.
template <bool P2, typename CT>
__global__ void k_einsum_anyk(const CT* __restrict__ A,
                              const CT* __restrict__ B,
                              CT* __restrict__ C, u64 nout, GatherMap omap,
                              GatherMap kmap, u64 K) {
  using RT = decltype(CT{}.x);
  for (u64 p = blockIdx.x * (u64)blockDim.x + threadIdx.x; p < nout;
       p += gridDim.x * (u64)blockDim.x) {
    i64 oa, ob;
    gather2<P2>(omap, p, oa, ob);
    RT re = 0, im = 0;
    for (u64 k = 0; k < K; ++k) {
      i64 ka, kb;
      gather2<P2>(kmap, k, ka, kb);
      CT a = A[oa + ka];
      CT b = B[ob + kb];
      re = fma(a.x, b.x, fma(-a.y, b.y, re));
      im = fma(a.x, b.y, fma(a.y, b.x, im));
    }
    C[p] = CT{re, im};
  }
}

// Tiled bit-permutation copy for pow2 full-span permutes (the TTGT packs
// and unpack): dst[p] = src[spread(p)]. k_permute_ct reads src scattered
// (one 8/16 B element per lane); here the 6 lowest-src-stride bits are the
// lane index of a coalesced READ and the 6 lowest free dst bits the lane
// index of a coalesced WRITE, staged through a 64x64 XOR-swizzled LDS tile
// (64 KB c128 -> 2 blocks/CU).
// (TN_PERM_*, PermPerm and plan_permute_tile: step_plan.hpp)

template <typename CT>
__global__ __launch_bounds__(512) void k_permute_tile(
    const CT* __restrict__ src, CT* __restrict__ dst, PermPerm pp) {
  constexpr int AN = 1 << TN_PERM_AB, BN = 1 << TN_PERM_BB;
  __shared__ CT tile[AN * BN];
  __shared__ u64 sboffS[BN], sboffD[BN], saoffD[AN];
  const int tid = threadIdx.x;
  if (tid < BN) {
    u64 os = 0, od = 0;
    for (int i = 0; i < TN_PERM_BB; ++i)
      if (tid >> i & 1) {
        os += pp.bS[i];
        od += pp.bD[i];
      }
    sboffS[tid] = os;
    sboffD[tid] = od;
  } else if (tid < BN + AN) {
    const int a = tid - BN;
    u64 od = 0;
    for (int i = 0; i < TN_PERM_AB; ++i)
      if (a >> i & 1) od += pp.aD[i];
    saoffD[a] = od;
  }
  u64 baseS = 0, baseD = 0;
  {
    unsigned r = blockIdx.x;
    for (int i = 0; i < pp.rbits; ++i) {
      if (r & 1) {
        baseS += pp.restS[i];
        baseD += pp.restD[i];
      }
      r >>= 1;
    }
  }
  __syncthreads();
  for (int e = tid; e < AN * BN; e += 512) {
    // lane ~ a: coalesced src reads
    const int a = e & (AN - 1), b = e >> TN_PERM_AB;
    tile[b * AN + ((a ^ b) & (AN - 1))] = src[baseS + sboffS[b] + (u64)a];
  }
  __syncthreads();
  for (int e = tid; e < AN * BN; e += 512) {
    // lane ~ b: coalesced dst writes
    const int b = e & (BN - 1), a = e >> TN_PERM_BB;
    dst[baseD + saoffD[a] + sboffD[b]] = tile[b * AN + ((a ^ b) & (AN - 1))];
  }
}

// fast path: both operands contiguous and identically ordered over the
// contracted legs (the final amplitude dot of two same-legs tensors) —
// pure streaming, no index gather.
template <typename CT>
__global__ void k_dot_partial_linear(const CT* __restrict__ A,
                                     const CT* __restrict__ B,
                                     double2* __restrict__ ws, u64 K) {
  __shared__ double sre[256], sim[256];
  double re = 0.0, im = 0.0;
  for (u64 k = blockIdx.x * (u64)blockDim.x + threadIdx.x; k < K;
       k += gridDim.x * (u64)blockDim.x) {
    CT a = A[k];
    CT b = B[k];
    re = fma((double)a.x, (double)b.x, fma(-(double)a.y, (double)b.y, re));
    im = fma((double)a.x, (double)b.y, fma((double)a.y, (double)b.x, im));
  }
  sre[threadIdx.x] = re;
  sim[threadIdx.x] = im;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if (threadIdx.x < (unsigned)s) {
      sre[threadIdx.x] += sre[threadIdx.x + s];
      sim[threadIdx.x] += sim[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) ws[blockIdx.x] = make_double2(sre[0], sim[0]);
}

// Tiled dot for a contracted index that is a pure bit-permutation between
// two contiguous pow2 operands (the final amplitude dot of rqc networks:
// both operands hold the same 2^30-ish legs in scrambled orders). A naive
// gather reads one side as random 16B accesses (~1.6 TB/s); here both
// operands are read coalesced and the scramble happens in LDS.
//   a-bits: the 6 lowest A bits (lane index, coalesced A reads)
//   b-bits: the 6 lowest B bits not among the a-bits (coalesced B reads)
//   rest  : the remaining bits (one block per combination)
// Each block stages its 64x64 B tile in LDS (64 KB -> 2 blocks/CU, so one
// block's loads overlap another's compute; the 128x64 variant measured
// 10.7 ms vs 6.2 ms for this at K=2^30 c128; XOR-swizzled so both the
// b-major writes and a-major reads are bank-conflict-free), then streams A.
// (TN_DOT_TILE_* and DotPerm: step_plan.hpp)

template <typename CT, int BB>
__global__ __launch_bounds__(512) void k_dot_tile(const CT* __restrict__ A,
                                                  const CT* __restrict__ B,
                                                  double2* __restrict__ ws,
                                                  DotPerm dp) {
  constexpr int NB = 1 << BB;
  __shared__ CT tile[NB * 64];
  __shared__ u64 sboffA[NB], sboffB[NB], saoffB[64];
  __shared__ double sred[16];
  const int tid = threadIdx.x;
  if (tid < NB) {
    u64 oa = 0, ob = 0;
    for (int i = 0; i < BB; ++i)
      if (tid >> i & 1) {
        oa += dp.bA[i];
        ob += dp.bB[i];
      }
    sboffA[tid] = oa;
    sboffB[tid] = ob;
  } else if (tid < NB + 64) {
    const int a = tid - NB;
    u64 ob = 0;
    for (int i = 0; i < TN_DOT_TILE_ABITS; ++i)
      if (a >> i & 1) ob += dp.aB[i];
    saoffB[a] = ob;
  }
  u64 baseA = 0, baseB = 0;
  {
    unsigned r = blockIdx.x;
    for (int i = 0; i < dp.rbits; ++i) {
      if (r & 1) {
        baseA += dp.restA[i];
        baseB += dp.restB[i];
      }
      r >>= 1;
    }
  }
  __syncthreads();
  for (int e = tid; e < NB * 64; e += 512) {
    const int b = e & (NB - 1), a = e >> BB;
    tile[b * 64 + (a ^ (b & 63))] = B[baseB + saoffB[a] + sboffB[b]];
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  double re = 0.0, im = 0.0;
  for (int b = wave; b < NB; b += 8) {
    const CT av = A[baseA + sboffA[b] + (u64)lane];
    const CT bv = tile[b * 64 + (lane ^ (b & 63))];
    re = fma((double)av.x, (double)bv.x, fma(-(double)av.y, (double)bv.y, re));
    im = fma((double)av.x, (double)bv.y, fma((double)av.y, (double)bv.x, im));
  }
  for (int s = 32; s > 0; s >>= 1) {
    re += __shfl_xor(re, s, 64);
    im += __shfl_xor(im, s, 64);
  }
  if (lane == 0) {
    sred[wave * 2] = re;
    sred[wave * 2 + 1] = im;
  }
  __syncthreads();
  if (tid == 0) {
    double tre = 0.0, tim = 0.0;
    for (int w = 0; w < 8; ++w) {
      tre += sred[w * 2];
      tim += sred[w * 2 + 1];
    }
    ws[blockIdx.x] = make_double2(tre, tim);
  }
}

template <bool P2, typename CT>
__global__ void k_dot_partial(const CT* __restrict__ A,
                              const CT* __restrict__ B,
                              double2* __restrict__ ws, u64 K, GatherMap kmap) {
  __shared__ double sre[256], sim[256];
  double re = 0.0, im = 0.0;
  for (u64 k = blockIdx.x * (u64)blockDim.x + threadIdx.x; k < K;
       k += gridDim.x * (u64)blockDim.x) {
    i64 ka, kb;
    gather2<P2>(kmap, k, ka, kb);
    CT a = A[ka];
    CT b = B[kb];
    re = fma((double)a.x, (double)b.x, fma(-(double)a.y, (double)b.y, re));
    im = fma((double)a.x, (double)b.y, fma((double)a.y, (double)b.x, im));
  }
  sre[threadIdx.x] = re;
  sim[threadIdx.x] = im;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if (threadIdx.x < (unsigned)s) {
      sre[threadIdx.x] += sre[threadIdx.x + s];
      sim[threadIdx.x] += sim[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) ws[blockIdx.x] = make_double2(sre[0], sim[0]);
}

template <typename CT>
__global__ void k_dot_finish(const double2* __restrict__ ws, CT* out,
                             int nblocks) {
  using RT = decltype(CT{}.x);
  __shared__ double sre[256], sim[256];
  double re = 0.0, im = 0.0;
  for (int i = threadIdx.x; i < nblocks; i += blockDim.x) {
    re += ws[i].x;
    im += ws[i].y;
  }
  sre[threadIdx.x] = re;
  sim[threadIdx.x] = im;
  __syncthreads();
  for (int s = blockDim.x / 2; s > 0; s >>= 1) {
    if (threadIdx.x < (unsigned)s) {
      sre[threadIdx.x] += sre[threadIdx.x + s];
      sim[threadIdx.x] += sim[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) *out = CT{(RT)sre[0], (RT)sim[0]};
}

// dst[p] = src[gather(p)] — pack / unpack / general permute (also serves the
// final-tensor Permutor, circuit_builder.rs:89-106, on device).
template <bool P2, typename CT>
__global__ void k_permute_ct(const CT* __restrict__ src,
                             CT* __restrict__ dst, u64 n, GatherMap map) {
  for (u64 p = blockIdx.x * (u64)blockDim.x + threadIdx.x; p < n;
       p += gridDim.x * (u64)blockDim.x) {
    dst[p] = src[gather1<P2>(map, p)];
  }
}

// --- complex GEMM, C[M,N] = A[M,K] @ B[K,N], interleaved c128, row-major ---
// 64x64 C tile per 256-thread block; linearized grid (tile = blockIdx.x,
// row tile = tile / col_tiles) so huge M or N never overflow grid dims.

#define GK 16  // (GT: step_plan.hpp)

template <typename CT>
__global__ __launch_bounds__(256) void k_zgemm_v1(
    const CT* __restrict__ A, const CT* __restrict__ B,
    CT* __restrict__ C, u64 M, u64 N, u64 K, unsigned col_tiles,
    unsigned tiles, u64 kchunk) {
  __shared__ CT As[GT][GK + 1];
  __shared__ CT Bs[GK][GT + 1];
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  // 32-bit tile decode (64-bit div emulation costs ~20 VGPRs)
  const unsigned tile = (unsigned)blockIdx.x % tiles;
  const unsigned slice = (unsigned)blockIdx.x / tiles;
  const u64 brow = (u64)(tile / col_tiles) * GT;
  const u64 bcol = (u64)(tile % col_tiles) * GT;
  const u64 kbeg = (u64)slice * kchunk;
  const u64 kend = (kbeg + kchunk < K) ? kbeg + kchunk : K;
  C += (u64)slice * M * N;  // slice 0 == C itself when kchunk == K
  CT acc[4][4];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) acc[i][j] = CT{0, 0};
  for (u64 k0 = kbeg; k0 < kend; k0 += GK) {
    for (int i = threadIdx.x; i < GT * GK; i += 256) {
      int r = i / GK, c = i % GK;
      As[r][c] = (brow + r < M && k0 + c < kend) ? A[(brow + r) * K + k0 + c]
                                                 : CT{0, 0};
    }
    for (int i = threadIdx.x; i < GK * GT; i += 256) {
      int r = i / GT, c = i % GT;
      Bs[r][c] = (k0 + r < kend && bcol + c < N) ? B[(k0 + r) * N + bcol + c]
                                                 : CT{0, 0};
    }
    __syncthreads();
    for (int kk = 0; kk < GK; ++kk) {
      CT a[4], b[4];
      for (int i = 0; i < 4; ++i) a[i] = As[ty * 4 + i][kk];
      for (int j = 0; j < 4; ++j) b[j] = Bs[kk][tx * 4 + j];
      for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
          acc[i][j].x = fma(a[i].x, b[j].x, fma(-a[i].y, b[j].y, acc[i][j].x));
          acc[i][j].y = fma(a[i].x, b[j].y, fma(a[i].y, b[j].x, acc[i][j].y));
        }
    }
    __syncthreads();
  }
  for (int i = 0; i < 4; ++i) {
    u64 r = brow + ty * 4 + i;
    if (r >= M) continue;
    for (int j = 0; j < 4; ++j) {
      u64 c = bcol + tx * 4 + j;
      if (c < N) C[r * N + c] = acc[i][j];
    }
  }
}

// MFMA f64 kernel: v_mfma_f64_16x16x4_f64, 8 waves per block, 128x64 tile
// (tile scan on the dominant rqc36 shape: 128x64/8-wave 58.7 TF/s vs
// 64x64/4-wave 56.2; deeper K-tiles and 128-wide tiles lose to occupancy;
// Gauss 3-mult lost on THIS planar-staged 8-wave layout, with no control of
// the register budget — scripts/zgemm_tune.hip REORDER == 2; on the glds
// staging with a 2x2-wave layout it wins, see k_zgemm_c128_glds_3m).
// Wave w owns C rows [w*16, w*16+16); its row slab is 4 column fragments of
// 16x16, each a {re, im} accumulator pair (4 f64 regs each). Per k-quad:
// 4 MFMAs per fragment (Cr += ArBr; Cr += (-Ai)Bi; Ci += ArBi; Ci += AiBr).
// LDS staging is planar with padded rows to avoid bank conflicts.
typedef double v4d __attribute__((ext_vector_type(4)));
typedef float v4f __attribute__((ext_vector_type(4)));

// Per-precision MFMA core. D-fragment row maps verified on hardware
// (scripts/mfma_repro.hip): f64 16x16x4 -> row = 4*reg + lane/16,
// f32 16x16x4 -> row = (lane/16)*4 + reg (they differ!).
template <typename RT>
struct MfmaCore;
template <>
struct MfmaCore<double> {
  using acc_t = v4d;
  static __device__ __forceinline__ acc_t mfma(double a, double b, acc_t c) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int crow(int lane, int r) {
    return 4 * r + lane / 16;
  }
};
template <>
struct MfmaCore<float> {
  using acc_t = v4f;
  static __device__ __forceinline__ acc_t mfma(float a, float b, acc_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ int crow(int lane, int r) {
    return (lane / 16) * 4 + r;
  }
};

// (MF_T x MF_TN tile, MF_K deep: step_plan.hpp)
#define MF_THREADS 512
#define A_LD 17  // padded row stride (elements) for the A tiles
#define B_LD 66  // padded row stride for the B tiles

template <typename CT>
__global__ __launch_bounds__(MF_THREADS) void k_zgemm_mfma(
    const CT* __restrict__ A, const CT* __restrict__ B,
    CT* __restrict__ C, u64 M, u64 N, u64 K, unsigned col_tiles,
    unsigned tiles, u64 kchunk) {
  using RT = decltype(CT{}.x);
  using Core = MfmaCore<RT>;
  using acc_t = typename Core::acc_t;
  __shared__ RT Ar[MF_T * A_LD];
  __shared__ RT Ai[MF_T * A_LD];
  __shared__ RT Br[MF_K * B_LD];
  __shared__ RT Bi[MF_K * B_LD];

  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  const unsigned tile = (unsigned)blockIdx.x % tiles;
  const unsigned slice = (unsigned)blockIdx.x / tiles;
  const u64 brow = (u64)(tile / col_tiles) * MF_T;
  const u64 bcol = (u64)(tile % col_tiles) * MF_TN;
  const u64 kbeg = (u64)slice * kchunk;
  const u64 kend = (kbeg + kchunk < K) ? kbeg + kchunk : K;
  C += (u64)slice * M * N;
  const bool interior = (brow + MF_T <= M) && (bcol + MF_TN <= N);

  acc_t cr[4], ci[4];
  for (int f = 0; f < 4; ++f) {
    cr[f] = acc_t{0, 0, 0, 0};
    ci[f] = acc_t{0, 0, 0, 0};
  }

  // operand map (both precisions): lane l holds A[i = l%16][k = l/16] and
  // B[k = l/16][j = l%16]; the D row map is per-precision (MfmaCore::crow).
  const int fi = lane % 16;
  const int fk = lane / 16;

  for (u64 k0 = kbeg; k0 < kend; k0 += MF_K) {
    for (int i = threadIdx.x; i < MF_T * MF_K; i += MF_THREADS) {
      int r = i / MF_K, c = i % MF_K;
      CT v = (brow + r < M && k0 + c < kend) ? A[(brow + r) * K + k0 + c]
                                             : CT{0, 0};
      Ar[r * A_LD + c] = v.x;
      Ai[r * A_LD + c] = v.y;
    }
    for (int i = threadIdx.x; i < MF_K * MF_TN; i += MF_THREADS) {
      int r = i / MF_TN, c = i % MF_TN;
      CT v = (k0 + r < kend && bcol + c < N) ? B[(k0 + r) * N + bcol + c]
                                             : CT{0, 0};
      Br[r * B_LD + c] = v.x;
      Bi[r * B_LD + c] = v.y;
    }
    __syncthreads();
    for (int kq = 0; kq < MF_K / 4; ++kq) {
      const int arow = wave * 16 + fi;
      const int ak = kq * 4 + fk;
      const RT ar = Ar[arow * A_LD + ak];
      const RT ai = Ai[arow * A_LD + ak];
      for (int f = 0; f < 4; ++f) {
        const int bcolf = f * 16 + fi;
        const RT br = Br[ak * B_LD + bcolf];
        const RT bi = Bi[ak * B_LD + bcolf];
        cr[f] = Core::mfma(ar, br, cr[f]);
        cr[f] = Core::mfma(-ai, bi, cr[f]);
        ci[f] = Core::mfma(ar, bi, ci[f]);
        ci[f] = Core::mfma(ai, br, ci[f]);
      }
    }
    __syncthreads();
  }

  const int ccol = lane % 16;
  for (int f = 0; f < 4; ++f) {
    for (int r = 0; r < 4; ++r) {
      u64 row = brow + wave * 16 + Core::crow(lane, r);
      u64 col = bcol + f * 16 + ccol;
      if (interior || (row < M && col < N))
        C[row * N + col] = CT{cr[f][r], ci[f][r]};
    }
  }
}


// c128 glds kernel: same 128x64 tile, but LDS-DMA staging into an XOR-
// swizzled interleaved image read back as single ds_read_b128 per operand
// element (re+im together). +20% over the planar-staged kernel on the
// dominant rqc36 shape (70.2-70.7 TF/s = 90% of the 78.6 TF/s f64 spec
// peak; scripts/zgemm_tune.hip — double-buffering loses to occupancy).
// Edge tiles and K-tails use a bounds-guarded staging loop writing the
// identical image (glds cannot mask out-of-range lanes).
__global__ __launch_bounds__(MF_THREADS) void k_zgemm_c128_glds(
    const double2* __restrict__ A, const double2* __restrict__ B,
    double2* __restrict__ C, u64 M, u64 N, u64 K, unsigned col_tiles,
    unsigned tiles, u64 kchunk) {
  constexpr int TM = MF_T, TN = MF_TN, KT = MF_K;
  constexpr int ASLOTS = TM * KT;
  __shared__ double2 As[ASLOTS];  // [r][c ^ (r & 15)]
  __shared__ double2 Bs[KT * TN]; // [k][j ^ ((k & 3) << 4)]
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  const unsigned tile = (unsigned)blockIdx.x % tiles;
  const unsigned slice = (unsigned)blockIdx.x / tiles;
  const u64 brow = (u64)(tile / col_tiles) * TM;
  const u64 bcol = (u64)(tile % col_tiles) * TN;
  const u64 kbeg = (u64)slice * kchunk;
  const u64 kend = (kbeg + kchunk < K) ? kbeg + kchunk : K;
  C += (u64)slice * M * N;
  const bool interior = (brow + TM <= M) && (bcol + TN <= N);

  v4d cr[4], ci[4];
  for (int f = 0; f < 4; ++f) {
    cr[f] = v4d{0, 0, 0, 0};
    ci[f] = v4d{0, 0, 0, 0};
  }
  const int fi = lane % 16;

  for (u64 k0 = kbeg; k0 < kend; k0 += KT) {
    if (interior && k0 + KT <= kend) {
      // glds: LDS dst = wave-uniform base + lane*16; per-lane SOURCE
      // pre-swizzled so the image lands linearly.
      for (int piece = 0; piece < 4; ++piece) {
        int base = (wave * 4 + piece) * 64;
        int i = base + lane;
        int r = i / KT, c_sw = i % KT;
        int c = c_sw ^ (r & 15);
        const double2* src = &A[(brow + r) * K + k0 + c];
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)src,
            (__attribute__((address_space(3))) void*)&As[base], 16, 0, 0);
      }
      for (int piece = 0; piece < 2; ++piece) {
        int base = piece * 512 + wave * 64;
        int j = base + lane;
        int k = j / TN, col_sw = j % TN;
        int col = col_sw ^ ((k & 3) << 4);
        const double2* src = &B[(k0 + k) * N + bcol + col];
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)src,
            (__attribute__((address_space(3))) void*)&Bs[base], 16, 0, 0);
      }
    } else {
      for (int i = threadIdx.x; i < TM * KT; i += MF_THREADS) {
        int r = i / KT, c = i % KT;
        double2 v = (brow + r < M && k0 + c < kend)
                        ? A[(brow + r) * K + k0 + c]
                        : make_double2(0.0, 0.0);
        As[r * KT + (c ^ (r & 15))] = v;
      }
      for (int i = threadIdx.x; i < KT * TN; i += MF_THREADS) {
        int k = i / TN, col = i % TN;
        double2 v = (k0 + k < kend && bcol + col < N)
                        ? B[(k0 + k) * N + bcol + col]
                        : make_double2(0.0, 0.0);
        Bs[k * TN + (col ^ ((k & 3) << 4))] = v;
      }
    }
    __syncthreads();  // carries vmcnt(0): drains the LDS-DMAs
    for (int kq = 0; kq < KT / 4; ++kq) {
      const int arow = wave * 16 + fi;
      const int ak = kq * 4 + (lane / 16);
      double2 a = As[arow * KT + (ak ^ (arow & 15))];
      for (int f = 0; f < 4; ++f) {
        const int bcolf = f * 16 + fi;
        double2 b = Bs[ak * TN + (bcolf ^ ((ak & 3) << 4))];
        cr[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, cr[f], 0, 0, 0);
        cr[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a.y, b.y, cr[f], 0, 0, 0);
        ci[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.y, ci[f], 0, 0, 0);
        ci[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.x, ci[f], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  const int crow0 = wave * 16 + (lane / 16);
  const int ccol = lane % 16;
  for (int f = 0; f < 4; ++f) {
    for (int r = 0; r < 4; ++r) {
      u64 row = brow + crow0 + 4 * r;
      u64 col = bcol + f * 16 + ccol;
      if (interior || (row < M && col < N))
        C[row * N + col] = make_double2(cr[f][r], ci[f][r]);
    }
  }
}


// Pure-glds variant: no guarded branch in the loop (the in-loop fallback
// costs ~20% via register pressure). Launched only when M % 128 == 0,
// N % 64 == 0 and every K-slice is a whole number of 16-tiles.
__global__ __launch_bounds__(MF_THREADS) void k_zgemm_c128_glds_pure(
    const double2* __restrict__ A, const double2* __restrict__ B,
    double2* __restrict__ C, u64 M, u64 N, u64 K, unsigned col_tiles,
    unsigned tiles, u64 kchunk) {
  constexpr int TM = MF_T, TN = MF_TN, KT = MF_K;
  constexpr int ASLOTS = TM * KT;
  __shared__ double2 As[ASLOTS];
  __shared__ double2 Bs[KT * TN];
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  // 32-bit tile decode: 64-bit div emulation costs ~22 VGPRs and a whole
  // wave of occupancy (148 -> 126 VGPRs measured)
  const unsigned tile = (unsigned)blockIdx.x % tiles;
  const unsigned slice = (unsigned)blockIdx.x / tiles;
  const u64 brow = (u64)(tile / col_tiles) * TM;
  const u64 bcol = (u64)(tile % col_tiles) * TN;
  const u64 kbeg = (u64)slice * kchunk;
  const u64 kend = (kbeg + kchunk < K) ? kbeg + kchunk : K;
  C += (u64)slice * M * N;
  v4d cr[4], ci[4];
  for (int f = 0; f < 4; ++f) {
    cr[f] = v4d{0, 0, 0, 0};
    ci[f] = v4d{0, 0, 0, 0};
  }
  const int fi = lane % 16;
  for (u64 k0 = kbeg; k0 < kend; k0 += KT) {
    for (int piece = 0; piece < 4; ++piece) {
      int base = (wave * 4 + piece) * 64;
      int i = base + lane;
      int r = i / KT, c_sw = i % KT;
      int c = c_sw ^ (r & 15);
      const double2* src = &A[(brow + r) * K + k0 + c];
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)&As[base], 16, 0, 0);
    }
    for (int piece = 0; piece < 2; ++piece) {
      int base = piece * 512 + wave * 64;
      int j = base + lane;
      int k = j / TN, col_sw = j % TN;
      int col = col_sw ^ ((k & 3) << 4);
      const double2* src = &B[(k0 + k) * N + bcol + col];
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)&Bs[base], 16, 0, 0);
    }
    __syncthreads();
    for (int kq = 0; kq < KT / 4; ++kq) {
      const int arow = wave * 16 + fi;
      const int ak = kq * 4 + (lane / 16);
      double2 a = As[arow * KT + (ak ^ (arow & 15))];
      for (int f = 0; f < 4; ++f) {
        const int bcolf = f * 16 + fi;
        double2 b = Bs[ak * TN + (bcolf ^ ((ak & 3) << 4))];
        cr[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, cr[f], 0, 0, 0);
        cr[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a.y, b.y, cr[f], 0, 0, 0);
        ci[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.y, ci[f], 0, 0, 0);
        ci[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.x, ci[f], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  const int crow0 = wave * 16 + (lane / 16);
  const int ccol = lane % 16;
  for (int f = 0; f < 4; ++f)
    for (int r = 0; r < 4; ++r) {
      u64 row = brow + crow0 + 4 * r;
      u64 col = bcol + f * 16 + ccol;
      C[row * N + col] = make_double2(cr[f][r], ci[f][r]);
    }
}


// Gauss three-multiply (3M) variant of the pure-glds kernel: the GEMMs are
// MFMA-pipe-bound, so the work left to remove is the MFMAs themselves.
// Three accumulator sets P1 = Ar*Br, P2 = Ai*Bi, P3 = (Ar+Ai)*(Br+Bi) take 3
// v_mfma_f64_16x16x4_f64 per complex MAC instead of 4; the epilogue forms
// Cr = P1 - P2, Ci = (P3 - P1) - P2 (real-only operands give P3 == P1 and
// P2 == 0 bit for bit, hence Ci == 0.0 exactly). Same 128x64x16 tile,
// LDS-DMA staging, XOR-swizzled interleaved images, 32-bit tile decode and
// D-fragment row map as k_zgemm_c128_glds_pure, so tile and split-K
// arithmetic is unchanged. Layout: 4 waves as 2x2, each wave owns 64x32 =
// 4x2 fragments (3 sets x 8 fragments x 8 regs = 192 accumulator VGPRs), the
// operand sums a.x+a.y / b.x+b.y are formed once per k-quad in registers
// (6 ds_read_b128 + 6 v_add_f64 per 24 MFMAs). waves_per_eu(2, 2) pins the
// register budget at 256: launch_bounds alone lets the compiler take more,
// asking for 3+ waves spills. Shipped build (kernel-resource-usage remarks):
// 254 VGPRs, 0 AGPRs, no spill, 2 waves/SIMD, 48 KiB LDS -> 2 blocks/CU,
// the same blocks/CU and tile traffic as the 4M kernel.
// Staging addresses are a wave-uniform 64-bit base plus a 32-bit per-lane
// byte offset (keeps the 12 DMA addresses out of the register budget): the
// launcher must guarantee MF_T*K*16 and MF_K*N*16 fit in 32 bits, on top of
// the pure-shape conditions (M % 128 == 0, N % 64 == 0, K-slices whole
// 16-tiles). No guarded branch in the loop.
// PIPE selects the main loop. Serial (TN_GEMM3M_PIPE=0): per 16-deep K-tile
// 12 DMAs per wave, barrier, 96 MFMAs, barrier; a wave issues nothing while
// its tile is in flight. Pipelined (the default): the same 48 KiB as two
// halves of one 8-deep K-slab each, A [128][8] + B [8][64]; the DMAs of one
// half fly under the MFMAs of the other. Two barriers per 16-deep tile as
// before, the k order per accumulator is unchanged (bit-identical results),
// and both forms build to the same budget (254 / 256 VGPRs plain / scatter,
// no spill, 2 waves/SIMD, 49152 B).
// The pipelined half-step, in source order and, through sched_barrier(0)
// between the groups, in the assembly: barrier; the 6 fragment reads of the
// first k-quad; their 6 operand sums; the first quad's 24 MFMAs with the 6
// DMA pieces of the next slab behind MFMAs 2, 4, 8, 10, 14 and 16; then the
// second quad (6 reads, 6 sums, 24 MFMAs) in the compiler's order, fenced in
// front of the next barrier. The reads come before the DMAs so that the
// DMAs' issue does not stand in front of the LDS latency, and the DMAs go
// one by one under the MFMAs instead of six in a row in front of them; the
// last piece is 32 MFMAs old when the next barrier's vmcnt(0) asks for it.
// A finer schedule (fragments of the next row block read under each row
// block's 6 MFMAs, the barrier moved in front of the last row block) keeps
// each wave's own pipe fed without a gap and measured slower than this one:
// what covers a wave's two read gaps per half-step is the other block's wave
// on the same SIMD, and every instruction put between a wave's MFMAs costs
// it more than the gap does (profiles/r07_gemm3m_sched.md).
// The speed rests on these properties of the assembly (check them after a
// compiler change; kernel-resource-usage remarks and the loop body):
// exactly two s_barrier per loop trip, each with s_waitcnt vmcnt(0) in front
// and no other vmcnt wait; 6 global_load_lds and 48 MFMAs per half-step in
// the order above; <= 256 VGPRs, no scratch. The source pins the barriers,
// the first quad's reads, the DMAs and the first quad's MFMAs. It does not
// guarantee (1) that no vmcnt appears in front of a ds_read: hipcc keeps it
// out because this body is inlined into the kernels with __restrict__
// parameters (the alias scopes tell the DMAs' LDS writes from the ds_reads
// of the other half), and the same loop written straight into a __global__
// function drains the DMAs before the reads and runs slower than serial;
// (2) the order inside the second quad; (3) counted lgkmcnt(N) waits: hipcc
// turns every lgkmcnt into lgkmcnt(0) while an LDS-DMA is pending.
// SCATTER selects the epilogue only; the main loop is shared. The scatter
// epilogue stores C(row, col) at C[R(row) + Cc(col)] (ScatterMap,
// step_plan.hpp): a wave-uniform part from the tile origin plus a tile-local
// part from a 128-entry row table and a 64-entry column table, built in LDS
// over As once the main loop is done. Offsets are 64-bit throughout.
#define MF3_THREADS 256
#define MF3_FENCE() __builtin_amdgcn_sched_barrier(0)
template <bool SCATTER, bool PIPE>
__device__ __forceinline__ void zgemm_c128_3m_body(
    const double2* __restrict__ A, const double2* __restrict__ B,
    double2* __restrict__ C, u64 M, u64 N, u64 K, unsigned col_tiles,
    unsigned tiles, u64 kchunk, const ScatterMap* sm) {
  constexpr int TM = MF_T, TN = MF_TN, KT = MF_K;
  constexpr int WN = 2, FM = 4, FN = 2;
  constexpr int APIECES = TM * KT / MF3_THREADS;  // 8 glds per wave
  constexpr int BPIECES = KT * TN / MF3_THREADS;  // 4 glds per wave
  // scalar wave index in the pipelined loop: its staging bases live in SGPRs
  const int wave = PIPE ? __builtin_amdgcn_readfirstlane(threadIdx.x / 64)
                        : threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  const int wm = wave / WN, wn = wave % WN;
  const unsigned tile = (unsigned)blockIdx.x % tiles;
  const unsigned slice = (unsigned)blockIdx.x / tiles;
  const u64 brow = (u64)(tile / col_tiles) * TM;
  const u64 bcol = (u64)(tile % col_tiles) * TN;
  const u64 kbeg = (u64)slice * kchunk;
  const u64 kend = (kbeg + kchunk < K) ? kbeg + kchunk : K;
  C += (u64)slice * M * N;
  v4d p1[FM][FN], p2[FM][FN], p3[FM][FN];
  for (int i = 0; i < FM; ++i)
    for (int j = 0; j < FN; ++j) {
      p1[i][j] = v4d{0, 0, 0, 0};
      p2[i][j] = v4d{0, 0, 0, 0};
      p3[i][j] = v4d{0, 0, 0, 0};
    }
  const int fi = lane % 16;
  const int fk = lane / 16;
  double2* stagebuf;  // the staging array, reused by the scatter epilogue
  if constexpr (PIPE) {
    // one array: a second __shared__ object can make the compiler drain the
    // DMAs (vmcnt(0)) before every LDS read
    __shared__ double2 lds[TM * KT + KT * TN];
    stagebuf = lds;
    // Two halves of one 8-deep K-slab each: A [128][c ^ ((r >> 1) & 7)],
    // B [8][j ^ ((k & 3) << 4)], 24 KiB per half. A row is 128 B, so two
    // rows share a 256-B bank row; the XOR by (r >> 1) & 7 puts the 8 rows of
    // each parity of a 16-row fragment on 8 different slots whichever of the
    // two k values the ds_read_b128 lane group carries. While the MFMAs of
    // one half run, the DMAs of the other are in flight: the barrier that
    // opens a half-step waits (vmcnt(0)) for the DMAs issued under the
    // first k-quad of the half-step before and frees the half about to be
    // overwritten.
    constexpr int KH = KT / 2;
    constexpr int HALF = TM * KH + KH * TN;  // slots per half
    constexpr int AP = TM * KH / MF3_THREADS;  // 4 glds per wave
    constexpr int BP = KH * TN / MF3_THREADS;  // 2 glds per wave
    // per-lane source offsets, bytes: piece strides and the K advance are
    // wave-uniform and go into the scalar base. An A piece is 8 rows of 8
    // slots; row r = (wave * AP + piece) * 8 + lane / 8 gives (r >> 1) & 7 =
    // (lane / 16) ^ ((piece & 1) << 2), so odd pieces flip byte bit 6.
    const unsigned offA =
        ((unsigned)(lane / 8) * (unsigned)K + ((lane % 8) ^ (lane / 16))) *
        16u;
    const unsigned offB = (unsigned)(lane ^ (wave << 4)) * 16u;
    const char* Ab = (const char*)(A + (brow + (u64)wave * (AP * 8)) * K);
    const char* Bb = (const char*)(B + (u64)wave * N + bcol);
    const u64 apstride = (u64)8 * K * 16, bpstride = (u64)4 * N * 16;
    // DMA piece p of slab k into `half`: 0..3 are A's, 4..5 are B's
    auto dma = [&](int half, u64 k, int p) {
      double2* Ah = lds + half * HALF;
      double2* Bh = Ah + TM * KH;
      if (p < AP)
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(
                Ab + k * 16 + p * apstride + (offA ^ ((p & 1) << 6))),
            (__attribute__((address_space(3))) void*)&Ah[(wave * AP + p) * 64],
            16, 0, 0);
      else
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(
                Bb + k * N * 16 + (p - AP) * bpstride + offB),
            (__attribute__((address_space(3))) void*)&Bh[(p - AP) *
                                                             MF3_THREADS +
                                                         wave * 64],
            16, 0, 0);
    };
    auto rdA = [&](int half, int q, int i) {
      const int ak = q * 4 + fk;
      const int arow = (wm * FM + i) * 16 + fi;
      return lds[half * HALF + arow * KH + (ak ^ ((arow >> 1) & 7))];
    };
    auto rdB = [&](int half, int q, int j) {
      const int ak = q * 4 + fk;
      const int bcolf = (wn * FN + j) * 16 + fi;
      return lds[half * HALF + TM * KH + ak * TN + (bcolf ^ ((ak & 3) << 4))];
    };
    // One half-step. Every group of instructions up to the second k-quad
    // sits between two sched_barrier(0): the order below is the order in
    // the assembly.
    auto halfstep = [&](int half, u64 kn) {
      __syncthreads();  // this half has landed, the other one is free
      MF3_FENCE();
      double2 a[FM], b[FN];
      double as[FM], bs[FN];
      // the first k-quad's fragments before any DMA: the DMAs' issue does
      // not stand in front of the LDS latency
      for (int i = 0; i < FM; ++i) a[i] = rdA(half, 0, i);
      for (int j = 0; j < FN; ++j) b[j] = rdB(half, 0, j);
      MF3_FENCE();
      for (int i = 0; i < FM; ++i) as[i] = a[i].x + a[i].y;
      for (int j = 0; j < FN; ++j) bs[j] = b[j].x + b[j].y;
      MF3_FENCE();
      // first k-quad: 4 row blocks of 6 MFMAs; blocks 0-2 carry the 6 DMA
      // pieces of the next slab, one behind the 2nd and one behind the 4th
      // MFMA, so the last piece is 32 MFMAs old at the next vmcnt(0)
      for (int i = 0; i < FM; ++i) {
        const int d0 = i < 3 ? 2 * i : -1;
        p1[i][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i].x, b[0].x, p1[i][0], 0, 0, 0);
        p2[i][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i].y, b[0].y, p2[i][0], 0, 0, 0);
        MF3_FENCE();
        if (d0 >= 0) dma(half ^ 1, kn, d0);
        MF3_FENCE();
        p3[i][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[i], bs[0], p3[i][0], 0, 0, 0);
        p1[i][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i].x, b[1].x, p1[i][1], 0, 0, 0);
        MF3_FENCE();
        if (d0 >= 0) dma(half ^ 1, kn, d0 + 1);
        MF3_FENCE();
        p2[i][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i].y, b[1].y, p2[i][1], 0, 0, 0);
        p3[i][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[i], bs[1], p3[i][1], 0, 0, 0);
        MF3_FENCE();
      }
      // second k-quad: reads, sums, 24 MFMAs, in the compiler's order; the
      // fences on either side keep all of it behind the first quad and in
      // front of the next barrier
      for (int i = 0; i < FM; ++i) {
        a[i] = rdA(half, 1, i);
        as[i] = a[i].x + a[i].y;
      }
      for (int j = 0; j < FN; ++j) {
        b[j] = rdB(half, 1, j);
        bs[j] = b[j].x + b[j].y;
      }
      for (int i = 0; i < FM; ++i)
        for (int j = 0; j < FN; ++j) {
          p1[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i].x, b[j].x, p1[i][j], 0, 0, 0);
          p2[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i].y, b[j].y, p2[i][j], 0, 0, 0);
          p3[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[i], bs[j], p3[i][j], 0, 0, 0);
        }
      MF3_FENCE();
    };
    for (int p = 0; p < AP + BP; ++p) dma(0, kbeg, p);
    for (u64 k0 = kbeg; k0 < kend; k0 += KT) {
      halfstep(0, k0 + KH);
      // the last tile has nothing to prefetch: it stages its own first slab
      // again (in bounds, never read) so the loop stays uniform
      halfstep(1, k0 + KT < kend ? k0 + KT : k0);
    }
    __syncthreads();  // no DMA in flight and no reader left past this point
  } else {
    __shared__ double2 As[TM * KT];  // [r][c ^ (r & 15)]
    __shared__ double2 Bs[KT * TN];  // [k][j ^ ((k & 3) << 4)]
    stagebuf = As;
    for (u64 k0 = kbeg; k0 < kend; k0 += KT) {
      for (int piece = 0; piece < APIECES; ++piece) {
        int base = (wave * APIECES + piece) * 64;
        int i = base + lane;
        int r = i / KT, c_sw = i % KT;
        int c = c_sw ^ (r & 15);
        const char* src = (const char*)(A + brow * K + k0) +
                          (unsigned)(((unsigned)r * (unsigned)K + c) * 16u);
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)src,
            (__attribute__((address_space(3))) void*)&As[base], 16, 0, 0);
      }
      for (int piece = 0; piece < BPIECES; ++piece) {
        int base = piece * MF3_THREADS + wave * 64;
        int j = base + lane;
        int k = j / TN, col_sw = j % TN;
        int col = col_sw ^ ((k & 3) << 4);
        const char* src = (const char*)(B + k0 * N + bcol) +
                          (unsigned)(((unsigned)k * (unsigned)N + col) * 16u);
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)src,
            (__attribute__((address_space(3))) void*)&Bs[base], 16, 0, 0);
      }
      __syncthreads();  // carries vmcnt(0): drains the LDS-DMAs
      for (int kq = 0; kq < KT / 4; ++kq) {
        const int ak = kq * 4 + fk;
        double2 a[FM], b[FN];
        double as[FM], bs[FN];
        for (int i = 0; i < FM; ++i) {
          const int arow = (wm * FM + i) * 16 + fi;
          a[i] = As[arow * KT + (ak ^ (arow & 15))];
          as[i] = a[i].x + a[i].y;
        }
        for (int j = 0; j < FN; ++j) {
          const int bcolf = (wn * FN + j) * 16 + fi;
          b[j] = Bs[ak * TN + (bcolf ^ ((ak & 3) << 4))];
          bs[j] = b[j].x + b[j].y;
        }
        for (int i = 0; i < FM; ++i)
          for (int j = 0; j < FN; ++j) {
            p1[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i].x, b[j].x, p1[i][j], 0, 0, 0);
            p2[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i].y, b[j].y, p2[i][j], 0, 0, 0);
            p3[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(as[i], bs[j], p3[i][j], 0, 0, 0);
          }
      }
      __syncthreads();
    }
  }
  const int ccol = lane % 16;
  if constexpr (SCATTER) {
    // the loop's closing barrier has retired every read of the staging array
    u64* rowtab = (u64*)stagebuf;
    u64* coltab = rowtab + TM;
    const int t = threadIdx.x;
    if (t < TM + TN) {
      const bool isrow = t < TM;
      const int idx = isrow ? t : t - TM;
      const int nb = isrow ? 7 : 6;  // log2(TM), log2(TN)
      u64 off = 0;
      for (int b = 0; b < nb; ++b)
        if ((idx >> b) & 1) off += isrow ? sm->rstride[b] : sm->cstride[b];
      rowtab[t] = off;  // coltab follows rowtab
    }
    u64 base = 0;  // wave-uniform: the tile origin's destination offset
    for (int b = 7; b < sm->rbits; ++b)
      if ((brow >> b) & 1) base += sm->rstride[b];
    for (int b = 6; b < sm->cbits; ++b)
      if ((bcol >> b) & 1) base += sm->cstride[b];
    __syncthreads();
    for (int i = 0; i < FM; ++i)
      for (int j = 0; j < FN; ++j) {
        const u64 coff = base + coltab[(wn * FN + j) * 16 + ccol];
        for (int r = 0; r < 4; ++r) {
          const u64 roff = rowtab[(wm * FM + i) * 16 + (lane / 16) + 4 * r];
          C[roff + coff] = make_double2(
              p1[i][j][r] - p2[i][j][r],
              (p3[i][j][r] - p1[i][j][r]) - p2[i][j][r]);
        }
      }
  } else {
    for (int i = 0; i < FM; ++i)
      for (int j = 0; j < FN; ++j)
        for (int r = 0; r < 4; ++r) {
          u64 row = brow + (wm * FM + i) * 16 + (lane / 16) + 4 * r;
          u64 col = bcol + (wn * FN + j) * 16 + ccol;
          C[row * N + col] = make_double2(
              p1[i][j][r] - p2[i][j][r],
              (p3[i][j][r] - p1[i][j][r]) - p2[i][j][r]);
        }
  }
}

__global__ __launch_bounds__(MF3_THREADS)
__attribute__((amdgpu_waves_per_eu(2, 2))) void k_zgemm_c128_glds_3m(
    const double2* __restrict__ A, const double2* __restrict__ B,
    double2* __restrict__ C, u64 M, u64 N, u64 K, unsigned col_tiles,
    unsigned tiles, u64 kchunk) {
  zgemm_c128_3m_body<false, false>(A, B, C, M, N, K, col_tiles, tiles, kchunk,
                                   nullptr);
}

__global__ __launch_bounds__(MF3_THREADS)
__attribute__((amdgpu_waves_per_eu(2, 2))) void k_zgemm_c128_glds_3m_pipe(
    const double2* __restrict__ A, const double2* __restrict__ B,
    double2* __restrict__ C, u64 M, u64 N, u64 K, unsigned col_tiles,
    unsigned tiles, u64 kchunk) {
  zgemm_c128_3m_body<false, true>(A, B, C, M, N, K, col_tiles, tiles, kchunk,
                                  nullptr);
}

// Launched unsplit only (tiles == grid): the map covers one M x N output.
__global__ __launch_bounds__(MF3_THREADS)
__attribute__((amdgpu_waves_per_eu(2, 2))) void k_zgemm_c128_glds_3m_scatter(
    const double2* __restrict__ A, const double2* __restrict__ B,
    double2* __restrict__ C, u64 M, u64 N, u64 K, unsigned col_tiles,
    unsigned tiles, u64 kchunk, ScatterMap sm) {
  zgemm_c128_3m_body<true, false>(A, B, C, M, N, K, col_tiles, tiles, kchunk,
                                  &sm);
}

__global__ __launch_bounds__(MF3_THREADS)
__attribute__((amdgpu_waves_per_eu(2, 2)))
void k_zgemm_c128_glds_3m_scatter_pipe(
    const double2* __restrict__ A, const double2* __restrict__ B,
    double2* __restrict__ C, u64 M, u64 N, u64 K, unsigned col_tiles,
    unsigned tiles, u64 kchunk, ScatterMap sm) {
  zgemm_c128_3m_body<true, true>(A, B, C, M, N, K, col_tiles, tiles, kchunk,
                                 &sm);
}


// Gather-staged c128 glds GEMM: reads A and B straight through the TTGT
// pack PERMUTATION instead of from pre-packed copies — the pack kernels
// (and their read+write HBM traffic, ~54 GB per rqc36 contraction)
// disappear. Works because with pow2 dims the packed offset is SEPARABLE:
// src = rowOff(m) + khi(k0) + klo(c), where rowOff/klo are tiny per-block
// LDS tables built in the prologue and khi is a wave-uniform (SALU) sum
// per k-iteration; the per-lane staging address is then two adds, no
// heavier than the multiply it replaces. Everything else (XOR-swizzled
// interleaved LDS image, MFMA body, epilogue) is identical to
// k_zgemm_c128_glds_pure. Launched only for pure shapes (M%128 == 0,
// N%64 == 0, K%16 == 0) with all-pow2 dims. (GatherGemmMap: step_plan.hpp)
__global__ __launch_bounds__(MF_THREADS) void k_zgemm_c128_glds_gather(
    const double2* __restrict__ A, const double2* __restrict__ B,
    double2* __restrict__ C, u64 M, u64 N, u64 K, unsigned col_tiles,
    unsigned tiles, u64 kchunk, GatherGemmMap mA, GatherGemmMap mB) {
  constexpr int TM = MF_T, TN = MF_TN, KT = MF_K;
  __shared__ double2 As[TM * KT];
  __shared__ double2 Bs[KT * TN];
  __shared__ u64 rowOffA[TM];
  __shared__ u64 colOffB[TN];
  __shared__ u64 kloA[KT];
  __shared__ u64 kloB[KT];
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  const unsigned tile = (unsigned)blockIdx.x % tiles;
  const unsigned slice = (unsigned)blockIdx.x / tiles;
  const u64 brow = (u64)(tile / col_tiles) * TM;
  const u64 bcol = (u64)(tile % col_tiles) * TN;
  const u64 kbeg = (u64)slice * kchunk;
  const u64 kend = (kbeg + kchunk < K) ? kbeg + kchunk : K;
  C += (u64)slice * M * N;
  // offset tables (once per block)
  for (int t = threadIdx.x; t < TM + TN + 2 * KT; t += MF_THREADS) {
    if (t < TM) {
      u64 idx = brow + t, off = 0;
      for (int b = 0; b < mA.rbits; ++b)
        if ((idx >> b) & 1) off += mA.rstride[b];
      rowOffA[t] = off;
    } else if (t < TM + TN) {
      u64 idx = bcol + (t - TM), off = 0;
      for (int b = 0; b < mB.rbits; ++b)
        if ((idx >> b) & 1) off += mB.rstride[b];
      colOffB[t - TM] = off;
    } else if (t < TM + TN + KT) {
      int c = t - TM - TN;
      u64 off = 0;
      for (int b = 0; b < 4; ++b)
        if ((c >> b) & 1) off += mA.kstride[b];
      kloA[c] = off;
    } else {
      int c = t - TM - TN - KT;
      u64 off = 0;
      for (int b = 0; b < 4; ++b)
        if ((c >> b) & 1) off += mB.kstride[b];
      kloB[c] = off;
    }
  }
  __syncthreads();
  v4d cr[4], ci[4];
  for (int f = 0; f < 4; ++f) {
    cr[f] = v4d{0, 0, 0, 0};
    ci[f] = v4d{0, 0, 0, 0};
  }
  const int fi = lane % 16;
  for (u64 k0 = kbeg; k0 < kend; k0 += KT) {
    u64 khiA = 0, khiB = 0;
    for (int b = 4; b < mA.kbits; ++b)
      if ((k0 >> b) & 1) khiA += mA.kstride[b];
    for (int b = 4; b < mB.kbits; ++b)
      if ((k0 >> b) & 1) khiB += mB.kstride[b];
    const double2* Ak = A + khiA;
    const double2* Bk = B + khiB;
    for (int piece = 0; piece < 4; ++piece) {
      int base = (wave * 4 + piece) * 64;
      int i = base + lane;
      int r = i / KT, c_sw = i % KT;
      int c = c_sw ^ (r & 15);
      const double2* src = &Ak[rowOffA[r] + kloA[c]];
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)&As[base], 16, 0, 0);
    }
    for (int piece = 0; piece < 2; ++piece) {
      int base = piece * 512 + wave * 64;
      int j = base + lane;
      int k = j / TN, col_sw = j % TN;
      int col = col_sw ^ ((k & 3) << 4);
      const double2* src = &Bk[kloB[k] + colOffB[col]];
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)&Bs[base], 16, 0, 0);
    }
    __syncthreads();
    for (int kq = 0; kq < KT / 4; ++kq) {
      const int arow = wave * 16 + fi;
      const int ak = kq * 4 + (lane / 16);
      double2 a = As[arow * KT + (ak ^ (arow & 15))];
      for (int f = 0; f < 4; ++f) {
        const int bcolf = f * 16 + fi;
        double2 b = Bs[ak * TN + (bcolf ^ ((ak & 3) << 4))];
        cr[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, cr[f], 0, 0, 0);
        cr[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(-a.y, b.y, cr[f], 0, 0, 0);
        ci[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.y, ci[f], 0, 0, 0);
        ci[f] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.x, ci[f], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  const int crow0 = wave * 16 + (lane / 16);
  const int ccol = lane % 16;
  for (int f = 0; f < 4; ++f)
    for (int r = 0; r < 4; ++r) {
      u64 row = brow + crow0 + 4 * r;
      u64 col = bcol + f * 16 + ccol;
      C[row * N + col] = make_double2(cr[f][r], ci[f][r]);
    }
}


// c64 pure-glds kernel: one 16-byte LDS-DMA moves TWO float2 elements, so
// the swizzle works at pair granularity (8 pairs per 16-deep K row).
__global__ __launch_bounds__(MF_THREADS) void k_zgemm_c64_glds_pure(
    const float2* __restrict__ A, const float2* __restrict__ B,
    float2* __restrict__ C, u64 M, u64 N, u64 K, unsigned col_tiles,
    unsigned tiles, u64 kchunk) {
  constexpr int TM = MF_T, TN = MF_TN, KT = MF_K;
  __shared__ float2 As[TM * KT];  // [r][2*(cp ^ (r & 7)) + e]
  __shared__ float2 Bs[KT * TN];  // [k][2*(jp ^ ((k & 3) << 2)) + e]
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  const unsigned tile = (unsigned)blockIdx.x % tiles;
  const unsigned slice = (unsigned)blockIdx.x / tiles;
  const u64 brow = (u64)(tile / col_tiles) * TM;
  const u64 bcol = (u64)(tile % col_tiles) * TN;
  const u64 kbeg = (u64)slice * kchunk;
  const u64 kend = (kbeg + kchunk < K) ? kbeg + kchunk : K;
  C += (u64)slice * M * N;
  v4f cr[4], ci[4];
  for (int f = 0; f < 4; ++f) {
    cr[f] = v4f{0, 0, 0, 0};
    ci[f] = v4f{0, 0, 0, 0};
  }
  const int fi = lane % 16;
  for (u64 k0 = kbeg; k0 < kend; k0 += KT) {
    // A: 128x16 c64 = 1024 pair-slots; 8 waves x 2 pieces x 64 lanes
    for (int piece = 0; piece < 2; ++piece) {
      int base = (wave * 2 + piece) * 64;  // pair-slot base
      int i = base + lane;
      int r = i / (KT / 2), cp_sw = i % (KT / 2);
      int cp = cp_sw ^ (r & 7);
      const float2* src = &A[(brow + r) * K + k0 + 2 * cp];
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)&As[2 * base], 16, 0, 0);
    }
    // B: 16x64 c64 = 512 pair-slots; 8 waves x 1 piece
    {
      int base = wave * 64;
      int j = base + lane;
      int k = j / (TN / 2), jp_sw = j % (TN / 2);
      int jp = jp_sw ^ ((k & 3) << 2);
      const float2* src = &B[(k0 + k) * N + bcol + 2 * jp];
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) void*)src,
          (__attribute__((address_space(3))) void*)&Bs[2 * base], 16, 0, 0);
    }
    __syncthreads();
    for (int kq = 0; kq < KT / 4; ++kq) {
      const int arow = wave * 16 + fi;
      const int ak = kq * 4 + (lane / 16);
      float2 a = As[arow * KT + 2 * ((ak / 2) ^ (arow & 7)) + (ak & 1)];
      for (int f = 0; f < 4; ++f) {
        const int bcolf = f * 16 + fi;
        float2 b = Bs[ak * TN + 2 * ((bcolf / 2) ^ ((ak & 3) << 2)) +
                      (bcolf & 1)];
        cr[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, cr[f], 0, 0, 0);
        cr[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(-a.y, b.y, cr[f], 0, 0, 0);
        ci[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.y, ci[f], 0, 0, 0);
        ci[f] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.x, ci[f], 0, 0, 0);
      }
    }
    __syncthreads();
  }
  const int crow0 = wave * 16 + (lane / 16) * 4;  // f32 D map: (l/16)*4+r
  const int ccol = lane % 16;
  for (int f = 0; f < 4; ++f)
    for (int r = 0; r < 4; ++r) {
      u64 row = brow + crow0 + r;
      u64 col = bcol + f * 16 + ccol;
      C[row * N + col] = make_float2(cr[f][r], ci[f][r]);
    }
}

// split-K reduce: C[p] = sum over slices of ws[s][p]
template <typename CT>
__global__ void k_splitk_reduce(const CT* __restrict__ ws,
                                CT* __restrict__ C, u64 nout, int slices) {
  using RT = decltype(CT{}.x);
  for (u64 p = blockIdx.x * (u64)blockDim.x + threadIdx.x; p < nout;
       p += gridDim.x * (u64)blockDim.x) {
    RT re = 0, im = 0;
    for (int s = 0; s < slices; ++s) {
      CT v = ws[(u64)s * nout + p];
      re += v.x;
      im += v.y;
    }
    C[p] = CT{re, im};
  }
}

// Batched MFMA GEMM (TN_BATCH_GEMM): C[b] = A[b] @ B[b] for every batch
// element in ONE launch, over packed [batch][M][K], [batch][K][N] ->
// [batch][M][N]; no strides inside. Modelled on k_zgemm_mfma (same operand
// and D-fragment maps through MfmaCore, same planar padded LDS image, same
// bounds-guarded staging and store), with a 64x64 tile and four waves: the
// scan above k_zgemm_mfma has 64x64 within 5% of 128x64 on big shapes; on the
// small elements this class exists for (fewer than 256 tiles, often one) it
// halves the row padding. Block = (element, tile): tile = blockIdx.x % tiles,
// so a workgroup never straddles two elements. Ragged M, N and K are zero-
// filled in staging (K needs no multiple of 4) and guarded in the store.
#define BG_THREADS 256  // (BG_T: step_plan.hpp)
template <typename CT>
__global__ __launch_bounds__(BG_THREADS) void k_zgemm_batched(
    const CT* __restrict__ A, const CT* __restrict__ B, CT* __restrict__ C,
    u64 M, u64 N, u64 K, unsigned col_tiles, unsigned tiles) {
  using RT = decltype(CT{}.x);
  using Core = MfmaCore<RT>;
  using acc_t = typename Core::acc_t;
  __shared__ RT Ar[BG_T * A_LD];
  __shared__ RT Ai[BG_T * A_LD];
  __shared__ RT Br[MF_K * B_LD];
  __shared__ RT Bi[MF_K * B_LD];

  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  const unsigned elem = (unsigned)blockIdx.x / tiles;
  const unsigned tile = (unsigned)blockIdx.x % tiles;
  const u64 brow = (u64)(tile / col_tiles) * BG_T;
  const u64 bcol = (u64)(tile % col_tiles) * BG_T;
  A += (u64)elem * M * K;
  B += (u64)elem * K * N;
  C += (u64)elem * M * N;

  acc_t cr[4], ci[4];
  for (int f = 0; f < 4; ++f) {
    cr[f] = acc_t{0, 0, 0, 0};
    ci[f] = acc_t{0, 0, 0, 0};
  }
  const int fi = lane % 16;
  const int fk = lane / 16;

  for (u64 k0 = 0; k0 < K; k0 += MF_K) {
    for (int i = threadIdx.x; i < BG_T * MF_K; i += BG_THREADS) {
      int r = i / MF_K, c = i % MF_K;
      CT v = (brow + r < M && k0 + c < K) ? A[(brow + r) * K + k0 + c]
                                          : CT{0, 0};
      Ar[r * A_LD + c] = v.x;
      Ai[r * A_LD + c] = v.y;
    }
    for (int i = threadIdx.x; i < MF_K * BG_T; i += BG_THREADS) {
      int r = i / BG_T, c = i % BG_T;
      CT v = (k0 + r < K && bcol + c < N) ? B[(k0 + r) * N + bcol + c]
                                          : CT{0, 0};
      Br[r * B_LD + c] = v.x;
      Bi[r * B_LD + c] = v.y;
    }
    __syncthreads();
    for (int kq = 0; kq < MF_K / 4; ++kq) {
      const int arow = wave * 16 + fi;
      const int ak = kq * 4 + fk;
      const RT ar = Ar[arow * A_LD + ak];
      const RT ai = Ai[arow * A_LD + ak];
      for (int f = 0; f < 4; ++f) {
        const int bcolf = f * 16 + fi;
        const RT br = Br[ak * B_LD + bcolf];
        const RT bi = Bi[ak * B_LD + bcolf];
        cr[f] = Core::mfma(ar, br, cr[f]);
        cr[f] = Core::mfma(-ai, bi, cr[f]);
        ci[f] = Core::mfma(ar, bi, ci[f]);
        ci[f] = Core::mfma(ai, br, ci[f]);
      }
    }
    __syncthreads();
  }

  const int ccol = lane % 16;
  for (int f = 0; f < 4; ++f) {
    for (int r = 0; r < 4; ++r) {
      u64 row = brow + wave * 16 + Core::crow(lane, r);
      u64 col = bcol + f * 16 + ccol;
      if (row < M && col < N) C[row * N + col] = CT{cr[f][r], ci[f][r]};
    }
  }
}

// ---------------------------------------------------------------------------
// host-side planning
// ---------------------------------------------------------------------------

static void ensure_mempool(int device) {
  static bool done[64] = {};
  if (device >= 0 && device < 64 && !done[device]) {
    hipMemPool_t pool;
    if (hipDeviceGetDefaultMemPool(&pool, device) == hipSuccess) {
      uint64_t threshold = UINT64_MAX;
      (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold,
                                   &threshold);
    }
    done[device] = true;
  }
}

struct StepStats {
  int kind;  // 0 smallk/anyk, 1 dot, 2 gemm, 3 gemm+unpack
  u64 m, n, k;
  hipEvent_t gemm_ev0 = nullptr;  // when set, record around the GEMM launch
  hipEvent_t gemm_ev1 = nullptr;
};

// --- device arena: one reserved slab, host-side first-fit bookkeeping ---
// Reuse is stream-ordered (all users launch on one stream), so a freed
// block can be handed out immediately: the consuming kernels are ordered
// behind the producing ones. Avoids hipMallocAsync's per-allocation page
// mapping, which costs seconds per contraction at 30-70 GB intermediates.
struct Arena {
  char* base = nullptr;
  size_t size = 0;
  struct Block {
    size_t off, sz;
    bool free;
  };
  std::vector<Block> blocks;

  int reserve(size_t bytes) {
    if (base) return 0;
    // never try to reserve more than the device can hold: clamp to 90% of
    // free memory so per-step spill allocations still have headroom
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > 0) {
      size_t cap = free_b - free_b / 10;
      if (bytes > cap) bytes = cap;
    }
    if (hipMalloc((void**)&base, bytes) != hipSuccess) {
      (void)hipGetLastError();  // swallow the sticky OOM; caller recovers
      return -1;
    }
    size = bytes;
    blocks = {{0, bytes, true}};
    return 0;
  }
  void* alloc(size_t bytes) {
    if (!base) return nullptr;
    bytes = (bytes + 255) & ~(size_t)255;
    for (size_t i = 0; i < blocks.size(); ++i) {
      if (blocks[i].free && blocks[i].sz >= bytes) {
        size_t off = blocks[i].off;
        if (blocks[i].sz > bytes) {
          blocks.insert(blocks.begin() + i + 1,
                        {off + bytes, blocks[i].sz - bytes, true});
        }
        blocks[i].sz = bytes;
        blocks[i].free = false;
        return base + off;
      }
    }
    return nullptr;  // exhausted -> caller falls back
  }
  bool owns(const void* p) const {
    return base && p >= base && p < base + size;
  }
  void release(void* p) {
    size_t off = (char*)p - base;
    for (size_t i = 0; i < blocks.size(); ++i) {
      if (blocks[i].off == off) {
        blocks[i].free = true;
        // merge with next, then previous
        if (i + 1 < blocks.size() && blocks[i + 1].free) {
          blocks[i].sz += blocks[i + 1].sz;
          blocks.erase(blocks.begin() + i + 1);
        }
        if (i > 0 && blocks[i - 1].free) {
          blocks[i - 1].sz += blocks[i].sz;
          blocks.erase(blocks.begin() + i);
        }
        return;
      }
    }
  }
  void destroy() {
    if (base) (void)hipFree(base);
    base = nullptr;
    blocks.clear();
  }
};

// workspace allocation context threaded through the einsum implementation
struct WsCtx {
  Arena* arena = nullptr;  // optional
  hipStream_t stream = nullptr;
  // stream-capture mode (hipGraph): non-arena allocations are refused and
  // poison the graph (hipMalloc is illegal mid-capture, and its pointers
  // would dangle on replay); frees must be deferred past EndCapture (hipFree
  // device-syncs, which is illegal mid-capture)
  bool capturing = false;
  bool spilled = false;
  std::vector<void*>* deferred = nullptr;
  // pack-pipeline stream (null = pipelining off): pack permutes of the
  // TTGT route may run K-window-chunked on this stream, overlapped with
  // the window GEMMs on `stream`
  hipStream_t stream2 = nullptr;
  // deferred event destruction (capture mode); null = destroy immediately
  std::vector<hipEvent_t>* events = nullptr;
};

// Non-arena workspace uses plain hipMalloc, NOT hipMallocAsync: on this
// ROCm stack the stream-ordered pool intermittently loses kernel writes to
// freshly-expanded pool pages (trailing rows of a GEMM output read back as
// zeros even with AMD_SERIALIZE_KERNEL=3; plain hipMalloc is always clean).
// The hot path (tn_net) uses the Arena slab, so the sync cost lands only on
// the standalone einsum entry points and the arena-exhaustion fallback.
static int ws_alloc(WsCtx& ctx, void** p, size_t bytes) {
  if (ctx.arena) {
    *p = ctx.arena->alloc(bytes);
    if (*p) return TN_OK;
  }
  if (ctx.capturing) {
    // Outside the arena there is only hipMalloc, which a thread may not call
    // while its stream captures: the runtime invalidates the capture and the
    // stream stays in capture mode past EndCapture. Report the spill; the
    // caller drops this capture and runs normally.
    ctx.spilled = true;
    g_last_error = "arena exhausted under stream capture";
    return TN_ERR_OOM;
  }
  if (hipMalloc(p, bytes) != hipSuccess) {
    (void)hipGetLastError();  // don't leave a sticky OOM for launch checks
    size_t fb = 0, tb = 0;
    (void)hipMemGetInfo(&fb, &tb);
    char buf[192];
    snprintf(buf, sizeof buf,
             "device allocation failed (%zu bytes; %zu free of %zu; arena %s)",
             bytes, fb, tb, ctx.arena ? "exhausted" : "absent");
    g_last_error = buf;
    return TN_ERR_OOM;
  }
  return TN_OK;
}

static void ws_free(WsCtx& ctx, void* p) {
  if (!p) return;
  if (ctx.arena && ctx.arena->owns(p)) {
    ctx.arena->release(p);
    return;
  }
  if (ctx.capturing && ctx.deferred) {
    ctx.deferred->push_back(p);
    return;
  }
  (void)hipFree(p);  // hipFree device-syncs before releasing the pages
}

// Launch the permute kernel plan_permute_tile (step_plan.hpp) chooses for a
// gather described by `ax`: the tiled bit permutation when it applies, else
// the index-gather permute.
template <typename CT>
static int launch_permute(const CT* src, CT* dst, u64 elems,
                          const std::vector<AxisInfo>& ax,
                          hipStream_t stream) {
  PermPerm pp;
  const int nr = plan_permute_tile(ax, elems, &pp);
  if (nr >= 0) {
    k_permute_tile<<<dim3(1u << nr), 512, 0, stream>>>(src, dst, pp);
  } else {
    GatherMap map;
    if (build_map(ax, &map)) FAILV(TN_ERR_INVALID, "rank too large");
    int blocks = grid_for(elems);
    if (map.pow2)
      k_permute_ct<true><<<blocks, 256, 0, stream>>>(src, dst, elems, map);
    else
      k_permute_ct<false><<<blocks, 256, 0, stream>>>(src, dst, elems, map);
  }
  HIP_CHECK(hipGetLastError());
  return TN_OK;
}

// Instantiated here, ahead of the einsum templates: the order in which the
// kernel templates are first used fixes their order in the code object, and
// the permute kernels come first in it.
template int launch_permute(const double2*, double2*, u64,
                            const std::vector<AxisInfo>&, hipStream_t);
template int launch_permute(const float2*, float2*, u64,
                            const std::vector<AxisInfo>&, hipStream_t);

// ---------------------------------------------------------------------------
// core einsum over device buffers; out is contiguous row-major in out order.
// plan_step (step_plan.hpp) decides everything that follows from shapes,
// strides, dtype and environment; the route functions below only allocate,
// launch and release.
// ---------------------------------------------------------------------------

// one planned step, as the route functions see it
template <typename CT>
struct Step {
  const StepPlan& p;
  const u64* out_shape;
  int out_nd;
  const Meta& A;
  const Meta& B;
  const CT* Adata;
  const CT* Bdata;
  CT* out;
  hipStream_t stream;
  WsCtx& ws;
  StepStats* stats;
};

// workspace block, released on every exit from its scope
template <typename T>
struct WsBlock {
  WsCtx& ws;
  T* p = nullptr;
  explicit WsBlock(WsCtx& w) : ws(w) {}
  WsBlock(const WsBlock&) = delete;
  ~WsBlock() { ws_free(ws, p); }
  int alloc(u64 bytes) {
    int rc = ws_alloc(ws, (void**)&p, bytes);
    if (rc) p = nullptr;
    return rc;
  }
};

// the pack pipeline's events: on every exit handed to ws.events (the walk
// destroys them when it is over), or destroyed here when there is no list
struct PipeEvents {
  WsCtx& ws;
  hipEvent_t e0 = nullptr, ep[16] = {};  // start; window w packed
  explicit PipeEvents(WsCtx& w) : ws(w) {}
  PipeEvents(const PipeEvents&) = delete;
  bool create(int P) {
    for (int w = -1; w < P; ++w) {
      hipEvent_t& e = w < 0 ? e0 : ep[w];
      if (hipEventCreate(&e) != hipSuccess) {
        e = nullptr;
        return false;
      }
    }
    return true;
  }
  void drop(hipEvent_t e) {
    if (e && ws.events)
      ws.events->push_back(e);
    else if (e)
      (void)hipEventDestroy(e);
  }
  ~PipeEvents() {
    drop(e0);
    for (hipEvent_t e : ep) drop(e);
  }
};

// ---- dot: scalar output, large K ----
template <typename CT>
static int run_dot(const Step<CT>& s) {
  const StepPlan& p = s.p;
  const int blocks = (int)p.dot_blocks;
  GatherMap kmap;
  if (p.dot_form == TN_DOT_GATHER &&
      build_map(k_axis_info(p, s.A, s.B), &kmap))
    FAILV(TN_ERR_INVALID, "rank too large");
  WsBlock<double2> wsbuf(s.ws);
  if (int rc = wsbuf.alloc(p.dot_blocks * sizeof(double2))) return rc;
  if (p.dot_form == TN_DOT_TILED) {
    // (finishes here, not below: the order in which the kernel templates
    // are first used fixes their order in the code object)
    k_dot_tile<CT, TN_DOT_TILE_BBITS><<<dim3((unsigned)p.dot_blocks), 512, 0,
                                         s.stream>>>(s.Adata, s.Bdata,
                                                     wsbuf.p, p.dp);
    k_dot_finish<<<1, 256, 0, s.stream>>>(wsbuf.p, s.out, blocks);
    HIP_CHECK(hipGetLastError());
    return TN_OK;
  }
  if (p.dot_form == TN_DOT_LINEAR)
    k_dot_partial_linear<<<blocks, 256, 0, s.stream>>>(s.Adata, s.Bdata,
                                                       wsbuf.p, p.k);
  else if (kmap.pow2)
    k_dot_partial<true><<<blocks, 256, 0, s.stream>>>(s.Adata, s.Bdata,
                                                      wsbuf.p, p.k, kmap);
  else
    k_dot_partial<false><<<blocks, 256, 0, s.stream>>>(s.Adata, s.Bdata,
                                                       wsbuf.p, p.k, kmap);
  k_dot_finish<<<1, 256, 0, s.stream>>>(wsbuf.p, s.out, blocks);
  HIP_CHECK(hipGetLastError());
  return TN_OK;
}

// ---- smallk / anyk: small K, or skinny GEMM shapes; also where a TTGT step
// goes when its workspace does not fit and the plan says gather_ok ----
// `lead`: out axes ahead of the element's own (a batched step's batch axes,
// which carry a stride in BOTH operands); nout counts them in
template <typename CT>
static int run_gather(const Step<CT>& s,
                      const std::vector<AxisInfo>& lead = {}) {
  const StepPlan& p = s.p;
  u64 nout = p.nout();
  const u64 K = p.k;
  if (s.stats) s.stats->kind = 0;
  for (const AxisInfo& ax : lead) nout *= ax.dim;
  const std::vector<AxisInfo> oax =
      gather_out_axis_info(p, s.out_shape, s.out_nd, s.A, s.B, lead);
  const std::vector<AxisInfo> kax = gather_k_axis_info(p, s.A, s.B);
  // the kernel, the grid and the maps' encoding: plan_gather_kernel
  const GatherChoice gc = plan_gather_kernel(oax, kax, nout, K);
  GatherMap omap, kmap;
  if (build_map(oax, &omap, gc.pow2) || build_map(kax, &kmap, gc.pow2))
    FAILV(TN_ERR_INVALID, "rank too large");
  const int blocks = gc.blocks;
  switch (gc.kernel) {
    case TN_GK_SMALLK_TBL:
      k_einsum_smallk_tbl<<<blocks, 256, 0, s.stream>>>(
          s.Adata, s.Bdata, s.out, nout, omap, kmap, (int)K);
      break;
    case TN_GK_SMALLK_P2:
      k_einsum_smallk<true><<<blocks, 256, 0, s.stream>>>(
          s.Adata, s.Bdata, s.out, nout, omap, kmap, (int)K);
      break;
    case TN_GK_SMALLK:
      k_einsum_smallk<false><<<blocks, 256, 0, s.stream>>>(
          s.Adata, s.Bdata, s.out, nout, omap, kmap, (int)K);
      break;
    case TN_GK_ANYK_P2:
      k_einsum_anyk<true><<<blocks, 256, 0, s.stream>>>(
          s.Adata, s.Bdata, s.out, nout, omap, kmap, K);
      break;
    default:  // TN_GK_ANYK
      k_einsum_anyk<false><<<blocks, 256, 0, s.stream>>>(
          s.Adata, s.Bdata, s.out, nout, omap, kmap, K);
      break;
  }
  HIP_CHECK(hipGetLastError());
  return TN_OK;
}

// ---- pipelined TTGT: window w's pack permutes run on stream2 while window
// w-1's GEMM runs on stream; the window GEMMs write split-K-style slices,
// reduced into Cg at the end. *done stays false when the window buffers or
// the events cannot be had: the caller then packs serially.
template <typename CT>
static int ttgt_pipelined(const Step<CT>& s, CT* Cg, bool* done) {
  const StepPlan& p = s.p;
  const Meta& A = s.A;
  const Meta& B = s.B;
  const u64 M = p.m, N = p.n, K = p.k, nout = p.nout();
  const int P = p.pipe_p, npre = p.pipe_npre;
  const u64 kc = p.pipe_kc;
  PipeEvents ev(s.ws);
  WsBlock<CT> slices(s.ws), Bwin(s.ws), Awin(s.ws);
  int rc_ = Awin.alloc(M * K * sizeof(CT));
  if (rc_ == TN_OK && p.pack_b) rc_ = Bwin.alloc(K * N * sizeof(CT));
  if (rc_ == TN_OK) rc_ = slices.alloc((u64)P * nout * sizeof(CT));
  if (rc_ != TN_OK || !ev.create(P)) return TN_OK;  // shortage
  // mixed-radix suffix products of the leading K legs (window digit x has
  // radix A.dims[k_a[x]])
  u64 sufA[16] = {};
  {
    u64 suf = 1;
    for (int x = npre - 1; x >= 0; --x) {
      sufA[x] = suf;
      suf *= A.dims[p.k_a[x]];
    }
  }
  HIP_CHECK(hipEventRecord(ev.e0, s.stream));
  HIP_CHECK(hipStreamWaitEvent(s.ws.stream2, ev.e0, 0));
  for (int w = 0; w < P; ++w) {
    // source offsets of window w
    u64 offA = 0, offB = 0;
    for (int x = 0; x < npre; ++x) {
      u64 digit = ((u64)w / sufA[x]) % A.dims[p.k_a[x]];
      offA += digit * (u64)A.strides[p.k_a[x]];
      offB += digit * (u64)B.strides[p.k_b[x]];
    }
    {
      int prc = launch_permute(s.Adata + offA, Awin.p + (u64)w * M * kc,
                               M * kc, window_a_axis_info(p, A, npre),
                               s.ws.stream2);
      if (prc) return prc;
    }
    if (p.pack_b) {
      int prc = launch_permute(s.Bdata + offB, Bwin.p + (u64)w * kc * N,
                               kc * N, window_b_axis_info(p, B, npre),
                               s.ws.stream2);
      if (prc) return prc;
    }
    HIP_CHECK(hipEventRecord(ev.ep[w], s.ws.stream2));
  }
  u64 tiles_w = (M / MF_T) * (N / MF_TN);
  if (s.stats && s.stats->gemm_ev0)
    HIP_CHECK(hipEventRecord(s.stats->gemm_ev0, s.stream));
  for (int w = 0; w < P; ++w) {
    HIP_CHECK(hipStreamWaitEvent(s.stream, ev.ep[w], 0));
    const CT* Aw = Awin.p + (u64)w * M * kc;
    const CT* Bw =
        p.pack_b ? Bwin.p + (u64)w * kc * N : s.Bdata + (u64)w * kc * N;
    CT* Cw = slices.p + (u64)w * nout;
    if constexpr (std::is_same_v<CT, double2>) {
      k_zgemm_c128_glds_pure<<<dim3((unsigned)tiles_w), MF_THREADS, 0,
                               s.stream>>>(Aw, Bw, Cw, M, N, kc,
                                           (unsigned)(N / MF_TN),
                                           (unsigned)tiles_w, kc);
    } else {
      k_zgemm_c64_glds_pure<<<dim3((unsigned)tiles_w), MF_THREADS, 0,
                              s.stream>>>(
          (const float2*)Aw, (const float2*)Bw, (float2*)Cw, M, N, kc,
          (unsigned)(N / MF_TN), (unsigned)tiles_w, kc);
    }
  }
  k_splitk_reduce<<<grid_for(nout), 256, 0, s.stream>>>(slices.p, Cg, nout,
                                                        P);
  if (s.stats && s.stats->gemm_ev1)
    HIP_CHECK(hipEventRecord(s.stats->gemm_ev1, s.stream));
  HIP_CHECK(hipGetLastError());
  *done = true;
  return TN_OK;
}

// ---- serial TTGT: pack (if needed) + GEMM into Cg. The pack blocks belong
// to the caller, which keeps them until the out permute is launched. Returns
// TN_ERR_OOM only when a pack buffer could not be had.
template <typename CT>
static int ttgt_serial(const Step<CT>& s, CT* Cg, WsBlock<CT>& packA,
                       WsBlock<CT>& packB) {
  const StepPlan& p = s.p;
  const u64 M = p.m, N = p.n, K = p.k, nout = p.nout();
  const CT* Ag = s.Adata;
  const CT* Bg = s.Bdata;
  auto pack = [&](const Meta& t, const AxisList& axes, u64 elems,
                  WsBlock<CT>& blk, const CT** src) -> int {
    if (int rc_ = blk.alloc(elems * sizeof(CT))) return rc_;
    if (int rc_ = launch_permute(*src, blk.p, elems, pack_axis_info(t, axes),
                                 s.stream))
      return rc_;
    *src = blk.p;
    return TN_OK;
  };
  if (!p.gather_gemm && p.pack_a)
    if (int rc_ = pack(s.A, p.a_axes, M * K, packA, &Ag)) return rc_;
  if (!p.gather_gemm && p.pack_b)
    if (int rc_ = pack(s.B, p.b_axes, K * N, packB, &Bg)) return rc_;

  const u64 tiles = p.row_tiles * p.col_tiles;
  u64 splitk = p.splitk, kchunk = p.kchunk;
  CT* gemm_out = Cg;
  WsBlock<CT> splitbuf(s.ws);
  if (splitk > 1) {
    int rc_ = splitbuf.alloc(splitk * nout * sizeof(CT));
    if (rc_ == TN_ERR_OOM) {
      splitk = 1;  // split-K is an optimization; run unsplit when tight
      kchunk = ((K + MF_K - 1) / MF_K) * MF_K;
    } else if (rc_) {
      return rc_;
    } else {
      gemm_out = splitbuf.p;
    }
  }
  const dim3 grid((unsigned)(tiles * splitk));
  const unsigned ct = (unsigned)p.col_tiles, nt = (unsigned)tiles;
  if (s.stats && s.stats->gemm_ev0)
    HIP_CHECK(hipEventRecord(s.stats->gemm_ev0, s.stream));
  // the c128 kernels exist for double2 only, the c64 ones for float2
  if constexpr (std::is_same_v<CT, double2>) {
    if (p.kernel == TN_GEMM_C128_GATHER)
      k_zgemm_c128_glds_gather<<<grid, MF_THREADS, 0, s.stream>>>(
          s.Adata, s.Bdata, gemm_out, M, N, K, ct, nt, kchunk, p.gmA, p.gmB);
    else if (p.kernel == TN_GEMM_C128_3M && p.scatter_out)
      (p.gemm_pipe ? k_zgemm_c128_glds_3m_scatter_pipe
                   : k_zgemm_c128_glds_3m_scatter)<<<grid, MF3_THREADS, 0,
                                                     s.stream>>>(
          Ag, Bg, gemm_out, M, N, K, ct, nt, kchunk, p.smap);
    else if (p.kernel == TN_GEMM_C128_3M)
      (p.gemm_pipe ? k_zgemm_c128_glds_3m_pipe
                   : k_zgemm_c128_glds_3m)<<<grid, MF3_THREADS, 0,
                                             s.stream>>>(
          Ag, Bg, gemm_out, M, N, K, ct, nt, kchunk);
    else if (p.kernel == TN_GEMM_C128_PURE)
      k_zgemm_c128_glds_pure<<<grid, MF_THREADS, 0, s.stream>>>(
          Ag, Bg, gemm_out, M, N, K, ct, nt, kchunk);
    else if (p.kernel == TN_GEMM_C128_GLDS)
      k_zgemm_c128_glds<<<grid, MF_THREADS, 0, s.stream>>>(
          Ag, Bg, gemm_out, M, N, K, ct, nt, kchunk);
  } else {
    if (p.kernel == TN_GEMM_C64_PURE)
      k_zgemm_c64_glds_pure<<<grid, MF_THREADS, 0, s.stream>>>(
          (const float2*)Ag, (const float2*)Bg, (float2*)gemm_out, M, N, K,
          ct, nt, kchunk);
    else if (p.kernel == TN_GEMM_MFMA)
      k_zgemm_mfma<<<grid, MF_THREADS, 0, s.stream>>>(Ag, Bg, gemm_out, M, N,
                                                      K, ct, nt, kchunk);
  }
  if (p.kernel == TN_GEMM_V1)
    k_zgemm_v1<<<grid, 256, 0, s.stream>>>(Ag, Bg, gemm_out, M, N, K, ct, nt,
                                           kchunk);
  if (splitk > 1)
    k_splitk_reduce<<<grid_for(nout), 256, 0, s.stream>>>(splitbuf.p, Cg,
                                                          nout, (int)splitk);
  if (s.stats && s.stats->gemm_ev1)
    HIP_CHECK(hipEventRecord(s.stats->gemm_ev1, s.stream));
  HIP_CHECK(hipGetLastError());
  return TN_OK;
}

// ---- TTGT: GEMM into `out`, or into a temporary C that is then permuted
// into out order ----
template <typename CT>
static int run_ttgt(const Step<CT>& s) {
  const StepPlan& p = s.p;
  // released in the order packA, packB, tmpC
  WsBlock<CT> tmpC(s.ws), packB(s.ws), packA(s.ws);
  CT* Cg = s.out;
  int rc_ = TN_OK;
  // (a scatter_out step is never pipelined or split: its GEMM stores
  // straight into out, in out order)
  const bool to_out = p.direct || p.scatter_out;
  if (!to_out) {
    rc_ = tmpC.alloc(p.nout() * sizeof(CT));
    Cg = tmpC.p;
  }
  bool pipelined = false;
  if (rc_ == TN_OK && p.pipe_p) rc_ = ttgt_pipelined(s, Cg, &pipelined);
  if (rc_ == TN_OK && !pipelined) rc_ = ttgt_serial(s, Cg, packA, packB);
  // the temporary C or a pack buffer doesn't fit -> run the shape through
  // the (slower) gather kernels instead of failing the whole contraction
  if (rc_ == TN_ERR_OOM && p.gather_ok) return run_gather(s);
  if (rc_ || to_out) return rc_;
  // permute tmp [M legs (out order)][N legs (out order)] -> out order
  const std::vector<AxisInfo> ax = out_axis_info(p, s.out_shape, s.out_nd);
  return launch_permute((const CT*)tmpC.p, s.out, p.nout(), ax, s.stream);
}

template <typename CT>
static int einsum_dev_impl(const u64* out_labels, const u64* out_shape,
                           int out_nd, const Meta& A, const Meta& B,
                           CT* out, hipStream_t stream, WsCtx& ws,
                           StepStats* stats) {
  StepPlan plan;
  std::string err;
  if (int rc = plan_step(std::is_same_v<CT, double2>, out_labels, out_shape,
                         out_nd, A, B, ws.stream2 != nullptr, &plan, &err)) {
    g_last_error = err;
    return rc;
  }
  if (stats) {
    stats->m = plan.m;
    stats->n = plan.n;
    stats->k = plan.k;
    stats->kind = plan.kind;
  }
  const Step<CT> s{plan, out_shape, out_nd, A, B, (const CT*)A.data,
                   (const CT*)B.data, out, stream, ws, stats};
  if (plan.route == TN_ROUTE_DOT) return run_dot(s);
  if (plan.route == TN_ROUTE_GATHER) return run_gather(s);
  return run_ttgt(s);
}

// ---- batch labels: plan_step_batched classifies, this dispatches ----

// GEMM class: pack what is not [batch][M][K] / [batch][K][N] already, one
// k_zgemm_batched launch, out permute when the caller's order is not
// [batch][M legs][N legs]. TN_ERR_OOM when a buffer cannot be had.
template <typename CT>
static int run_batch_gemm(const BatchPlan& p, const u64* out_shape, int out_nd,
                          const Meta& A, const Meta& B, CT* out,
                          hipStream_t stream, WsCtx& ws, StepStats* stats) {
  const StepPlan& e = p.ep;
  const u64 M = e.m, N = e.n, K = e.k, nout = p.batch * M * N;
  WsBlock<CT> tmpC(ws), packB(ws), packA(ws);
  const CT* Ag = (const CT*)A.data;
  const CT* Bg = (const CT*)B.data;
  CT* Cg = out;
  if (!e.direct) {
    if (int rc = tmpC.alloc(nout * sizeof(CT))) return rc;
    Cg = tmpC.p;
  }
  if (p.ws_pack_a) {
    if (int rc = packA.alloc(p.ws_pack_a)) return rc;
    if (int rc = launch_permute(
            Ag, packA.p, p.batch * M * K,
            batch_pack_axis_info(p, A, p.ba, p.Ae, e.a_axes), stream))
      return rc;
    Ag = packA.p;
  }
  if (p.ws_pack_b) {
    if (int rc = packB.alloc(p.ws_pack_b)) return rc;
    if (int rc = launch_permute(
            Bg, packB.p, p.batch * K * N,
            batch_pack_axis_info(p, B, p.bb, p.Be, e.b_axes), stream))
      return rc;
    Bg = packB.p;
  }
  const u64 tiles = p.row_tiles * p.col_tiles;
  if (stats && stats->gemm_ev0)
    HIP_CHECK(hipEventRecord(stats->gemm_ev0, stream));
  k_zgemm_batched<<<dim3((unsigned)(p.batch * tiles)), BG_THREADS, 0,
                    stream>>>(Ag, Bg, Cg, M, N, K, (unsigned)p.col_tiles,
                              (unsigned)tiles);
  if (stats && stats->gemm_ev1)
    HIP_CHECK(hipEventRecord(stats->gemm_ev1, stream));
  HIP_CHECK(hipGetLastError());
  if (e.direct) return TN_OK;
  return launch_permute((const CT*)tmpC.p, out, nout,
                        batch_out_axis_info(p, out_shape, out_nd), stream);
}

template <typename CT>
static int einsum_batched_impl(const u64* out_labels, const u64* out_shape,
                               int out_nd, const Meta& A, const Meta& B,
                               const u64* batch_labels, size_t nbatch,
                               CT* out, hipStream_t stream, WsCtx& ws,
                               StepStats* stats) {
  BatchPlan bp;
  std::string err;
  if (int rc = plan_step_batched(std::is_same_v<CT, double2>, out_labels,
                                 out_shape, out_nd, A, B, batch_labels, nbatch,
                                 ws.stream2 != nullptr, &bp, &err)) {
    g_last_error = err;
    return rc;
  }
  const StepPlan& e = bp.ep;
  if (stats) {
    stats->m = e.m;
    stats->n = e.n;
    stats->k = e.k;
    stats->kind = e.kind;
  }
  const u64* eshape = out_shape + bp.nb;
  const int end = out_nd - bp.nb;
  auto element = [&](u64 b) {
    const CT* Ab = (const CT*)A.data + batch_offset(bp, A, bp.ba, b);
    const CT* Bb = (const CT*)B.data + batch_offset(bp, B, bp.bb, b);
    const Step<CT> s{e, eshape, end, bp.Ae, bp.Be, Ab, Bb,
                     out + b * e.nout(), stream, ws, stats};
    if (e.route == TN_ROUTE_DOT) return run_dot(s);
    if (e.route == TN_ROUTE_GATHER) return run_gather(s);
    return run_ttgt(s);
  };
  if (bp.cls == TN_BATCH_NONE) return element(0);
  if (bp.cls == TN_BATCH_GATHER) {
    const Step<CT> s{e, eshape, end, bp.Ae, bp.Be, (const CT*)A.data,
                     (const CT*)B.data, out, stream, ws, stats};
    return run_gather(s, batch_lead_axis_info(bp, A, B));
  }
  if (bp.cls == TN_BATCH_GEMM) {
    int rc = run_batch_gemm(bp, out_shape, out_nd, A, B, out, stream, ws,
                            stats);
    // the batched buffers do not fit: LOOP needs 1/batch of the workspace
    if (rc != TN_ERR_OOM) return rc;
  }
  for (u64 b = 0; b < bp.batch; ++b)
    if (int rc = element(b)) return rc;
  return TN_OK;
}

// ---------------------------------------------------------------------------
// C API: device management + einsum entry points
// ---------------------------------------------------------------------------

static int g_device = 0;

extern "C" int tn_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

extern "C" int tn_set_device(int device) {
  HIP_CHECK(hipSetDevice(device));
  g_device = device;
  ensure_mempool(device);
  return TN_OK;
}

static int require_gpu() {
  if (tn_device_count() == 0)
    FAILV(TN_ERR_NO_GPU,
          "no AMD GPU present — tnc_hip has no CPU fallback by design");
  return TN_OK;
}

static int fill_meta(Meta* m, const u64* labels, const u64* shape,
                     const i64* strides, const void* data, size_t nd) {
  if (nd > TN_MAXR) FAILV(TN_ERR_INVALID, "rank %zu exceeds %d", nd, TN_MAXR);
  m->nd = (int)nd;
  i64 contig = 1;
  for (int i = (int)nd - 1; i >= 0; --i) {
    m->labels[i] = labels[i];
    m->dims[i] = shape[i];
    m->strides[i] = strides ? strides[i] : contig;
    contig *= (i64)shape[i];
  }
  m->data = (const double2*)data;
  return TN_OK;
}

// the batch labels of the *_batched entry points (null: the plain einsum)
struct BatchLabels {
  const u64* labels;
  size_t n;
};

template <typename CT>
static int einsum_dev_entry(const u64* out_labels, const u64* out_shape,
                            size_t out_ndim, const u64* a_labels,
                            const u64* a_shape, const i64* a_strides,
                            const void* a_dev, size_t a_ndim,
                            const u64* b_labels, const u64* b_shape,
                            const i64* b_strides, const void* b_dev,
                            size_t b_ndim, void* out_dev, void* stream,
                            const BatchLabels* batch = nullptr) {
  int rc = require_gpu();
  if (rc) return rc;
  Meta A, B;
  rc = fill_meta(&A, a_labels, a_shape, a_strides, a_dev, a_ndim);
  if (rc) return rc;
  rc = fill_meta(&B, b_labels, b_shape, b_strides, b_dev, b_ndim);
  if (rc) return rc;
  WsCtx ws{nullptr, (hipStream_t)stream};
  if (batch)
    return einsum_batched_impl<CT>(out_labels, out_shape, (int)out_ndim, A, B,
                                   batch->labels, batch->n, (CT*)out_dev,
                                   (hipStream_t)stream, ws, nullptr);
  return einsum_dev_impl<CT>(out_labels, out_shape, (int)out_ndim, A, B,
                             (CT*)out_dev, (hipStream_t)stream, ws, nullptr);
}

extern "C" int tn_einsum_c128_dev(const u64* out_labels, const u64* out_shape,
                                  size_t out_ndim, const u64* a_labels,
                                  const u64* a_shape, const i64* a_strides,
                                  const void* a_dev, size_t a_ndim,
                                  const u64* b_labels, const u64* b_shape,
                                  const i64* b_strides, const void* b_dev,
                                  size_t b_ndim, void* out_dev, void* stream) {
  return einsum_dev_entry<double2>(out_labels, out_shape, out_ndim, a_labels,
                                   a_shape, a_strides, a_dev, a_ndim, b_labels,
                                   b_shape, b_strides, b_dev, b_ndim, out_dev,
                                   stream);
}

extern "C" int tn_einsum_c64_dev(const u64* out_labels, const u64* out_shape,
                                 size_t out_ndim, const u64* a_labels,
                                 const u64* a_shape, const i64* a_strides,
                                 const void* a_dev, size_t a_ndim,
                                 const u64* b_labels, const u64* b_shape,
                                 const i64* b_strides, const void* b_dev,
                                 size_t b_ndim, void* out_dev, void* stream) {
  return einsum_dev_entry<float2>(out_labels, out_shape, out_ndim, a_labels,
                                  a_shape, a_strides, a_dev, a_ndim, b_labels,
                                  b_shape, b_strides, b_dev, b_ndim, out_dev,
                                  stream);
}

// the plan einsum_dev_impl would act on; no GPU needed, none touched
extern "C" int tn_plan_step(int dtype, const u64* out_labels,
                            const u64* out_shape, size_t out_ndim,
                            const u64* a_labels, const u64* a_shape,
                            const i64* a_strides, size_t a_ndim,
                            const u64* b_labels, const u64* b_shape,
                            const i64* b_strides, size_t b_ndim,
                            int has_stream2, tn_step_plan* plan) {
  if (!plan || (dtype != 0 && dtype != 1) || out_ndim > TN_MAXR)
    FAILV(TN_ERR_INVALID, "null plan, unknown dtype or rank over %d", TN_MAXR);
  Meta A, B;
  int rc = fill_meta(&A, a_labels, a_shape, a_strides, nullptr, a_ndim);
  if (rc) return rc;
  rc = fill_meta(&B, b_labels, b_shape, b_strides, nullptr, b_ndim);
  if (rc) return rc;
  StepPlan p;
  std::string err;
  rc = plan_step(dtype == 0, out_labels, out_shape, (int)out_ndim, A, B,
                 has_stream2 != 0, &p, &err);
  if (rc) {
    g_last_error = err;
    return rc;
  }
  *plan = p;
  return TN_OK;
}

extern "C" int tn_plan_layouts(int dtype, const u64* leaf_labels,
                               const u64* leaf_dims, const u64* leaf_nd,
                               size_t nleaves, const u64* pairs, size_t nsteps,
                               int32_t* scatter_out, u64* inline_pack_bytes) {
  if ((dtype != 0 && dtype != 1) || (nleaves && !leaf_nd) ||
      (nsteps && !pairs))
    FAILV(TN_ERR_INVALID, "unknown dtype or null leaves/pairs");
  std::vector<LayoutTensor> lt(nleaves);
  size_t at = 0;
  for (size_t x = 0; x < nleaves; ++x) {
    lt[x].labels.assign(leaf_labels + at, leaf_labels + at + leaf_nd[x]);
    lt[x].dims.assign(leaf_dims + at, leaf_dims + at + leaf_nd[x]);
    at += leaf_nd[x];
  }
  LayoutPlan lp;
  plan_layouts(dtype == 0, lt, pairs, nsteps, &lp);
  if (!lp.valid)
    FAILV(TN_ERR_INVALID, "invalid contraction path or rank over %d", TN_MAXR);
  for (size_t s = 0; s < nsteps; ++s) {
    if (scatter_out) scatter_out[s] = lp.scatter_out[s];
    if (inline_pack_bytes) inline_pack_bytes[s] = lp.inline_pack_bytes[s];
  }
  return TN_OK;
}

extern "C" int tn_plan_slices(int dtype, const u64* leaf_labels,
                              const u64* leaf_dims, const u64* leaf_nd,
                              size_t nleaves, const u64* pairs, size_t nsteps,
                              const u64* slice_labels, size_t nlabels,
                              u64* nassign, u64* reduced_nd, u64* strides) {
  if ((dtype != 0 && dtype != 1) || (nleaves && !leaf_nd) ||
      (nsteps && !pairs) || (nlabels && !slice_labels))
    FAILV(TN_ERR_INVALID, "unknown dtype or null leaves/pairs/slice labels");
  std::vector<LayoutTensor> lt(nleaves);
  size_t at = 0;
  for (size_t x = 0; x < nleaves; ++x) {
    lt[x].labels.assign(leaf_labels + at, leaf_labels + at + leaf_nd[x]);
    lt[x].dims.assign(leaf_dims + at, leaf_dims + at + leaf_nd[x]);
    at += leaf_nd[x];
  }
  SlicePlan sp;
  plan_slices(dtype == 0, lt, pairs, nsteps, slice_labels, nlabels, &sp);
  if (!sp.valid) FAILV(TN_ERR_INVALID, "%s", sp.err.c_str());
  if (nassign) *nassign = sp.count;
  for (size_t x = 0; reduced_nd && x < nleaves; ++x)
    reduced_nd[x] = sp.reduced[x].labels.size();
  if (strides) std::copy(sp.strides.begin(), sp.strides.end(), strides);
  return TN_OK;
}

static u64 span_elems(const u64* shape, const i64* strides, size_t nd) {
  // max linear offset + 1, assuming nonnegative strides
  u64 span = 1;
  for (size_t i = 0; i < nd; ++i)
    span += (shape[i] - 1) * (u64)(strides ? strides[i] : 0);
  if (!strides) {
    span = 1;
    for (size_t i = 0; i < nd; ++i) span *= shape[i];
  }
  return span;
}

template <typename CT>
static int einsum_host_entry(const u64* out_labels, const u64* out_shape,
                             size_t out_ndim, const u64* a_labels,
                             const u64* a_shape, const i64* a_strides,
                             const void* a_data, size_t a_ndim,
                             const u64* b_labels, const u64* b_shape,
                             const i64* b_strides, const void* b_data,
                             size_t b_ndim, void* out_data,
                             const BatchLabels* batch = nullptr) {
  int rc = require_gpu();
  if (rc) return rc;
  HIP_CHECK(hipSetDevice(g_device));
  ensure_mempool(g_device);
  const size_t es = sizeof(CT);
  if (a_strides)
    for (size_t i = 0; i < a_ndim; ++i)
      if (a_strides[i] < 0) FAILV(TN_ERR_INVALID, "negative strides");
  if (b_strides)
    for (size_t i = 0; i < b_ndim; ++i)
      if (b_strides[i] < 0) FAILV(TN_ERR_INVALID, "negative strides");
  u64 a_span = span_elems(a_shape, a_strides, a_ndim);
  u64 b_span = span_elems(b_shape, b_strides, b_ndim);
  u64 out_elems = 1;
  for (size_t i = 0; i < out_ndim; ++i) out_elems *= out_shape[i];
  void *da, *db, *dout;
  HIP_CHECK(hipMalloc(&da, a_span * es));
  HIP_CHECK(hipMalloc(&db, b_span * es));
  HIP_CHECK(hipMalloc(&dout, out_elems * es));
  HIP_CHECK(hipMemcpy(da, a_data, a_span * es, hipMemcpyHostToDevice));
  HIP_CHECK(hipMemcpy(db, b_data, b_span * es, hipMemcpyHostToDevice));
  rc = einsum_dev_entry<CT>(out_labels, out_shape, out_ndim, a_labels,
                            a_shape, a_strides, da, a_ndim, b_labels, b_shape,
                            b_strides, db, b_ndim, dout, nullptr, batch);
  if (rc == TN_OK) {
    HIP_CHECK(hipMemcpy(out_data, dout, out_elems * es,
                        hipMemcpyDeviceToHost));
  }
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dout);
  return rc;
}

extern "C" int tn_einsum_c128(const u64* out_labels, const u64* out_shape,
                              size_t out_ndim, const u64* a_labels,
                              const u64* a_shape, const i64* a_strides,
                              const void* a_data, size_t a_ndim,
                              const u64* b_labels, const u64* b_shape,
                              const i64* b_strides, const void* b_data,
                              size_t b_ndim, void* out_data) {
  return einsum_host_entry<double2>(out_labels, out_shape, out_ndim, a_labels,
                                    a_shape, a_strides, a_data, a_ndim,
                                    b_labels, b_shape, b_strides, b_data,
                                    b_ndim, out_data);
}

extern "C" int tn_einsum_c64(const u64* out_labels, const u64* out_shape,
                             size_t out_ndim, const u64* a_labels,
                             const u64* a_shape, const i64* a_strides,
                             const void* a_data, size_t a_ndim,
                             const u64* b_labels, const u64* b_shape,
                             const i64* b_strides, const void* b_data,
                             size_t b_ndim, void* out_data) {
  return einsum_host_entry<float2>(out_labels, out_shape, out_ndim, a_labels,
                                   a_shape, a_strides, a_data, a_ndim,
                                   b_labels, b_shape, b_strides, b_data,
                                   b_ndim, out_data);
}

// --- batch labels: C API ----------------------------------------------------

#define TN_EINSUM_ARGS                                                       \
  const u64 *out_labels, const u64 *out_shape, size_t out_ndim,              \
      const u64 *a_labels, const u64 *a_shape, const i64 *a_strides,         \
      const void *a_data, size_t a_ndim, const u64 *b_labels,                \
      const u64 *b_shape, const i64 *b_strides, const void *b_data,          \
      size_t b_ndim, const u64 *batch_labels, size_t nbatch
#define TN_EINSUM_PASS                                                       \
  out_labels, out_shape, out_ndim, a_labels, a_shape, a_strides, a_data,     \
      a_ndim, b_labels, b_shape, b_strides, b_data, b_ndim

extern "C" int tn_einsum_c128_batched(TN_EINSUM_ARGS, void* out_data) {
  if (nbatch && !batch_labels) FAILV(TN_ERR_INVALID, "null batch labels");
  const BatchLabels bl{batch_labels, nbatch};
  return einsum_host_entry<double2>(TN_EINSUM_PASS, out_data, &bl);
}

extern "C" int tn_einsum_c64_batched(TN_EINSUM_ARGS, void* out_data) {
  if (nbatch && !batch_labels) FAILV(TN_ERR_INVALID, "null batch labels");
  const BatchLabels bl{batch_labels, nbatch};
  return einsum_host_entry<float2>(TN_EINSUM_PASS, out_data, &bl);
}

extern "C" int tn_einsum_c128_batched_dev(TN_EINSUM_ARGS, void* out_dev,
                                          void* stream) {
  if (nbatch && !batch_labels) FAILV(TN_ERR_INVALID, "null batch labels");
  const BatchLabels bl{batch_labels, nbatch};
  return einsum_dev_entry<double2>(TN_EINSUM_PASS, out_dev, stream, &bl);
}

extern "C" int tn_einsum_c64_batched_dev(TN_EINSUM_ARGS, void* out_dev,
                                         void* stream) {
  if (nbatch && !batch_labels) FAILV(TN_ERR_INVALID, "null batch labels");
  const BatchLabels bl{batch_labels, nbatch};
  return einsum_dev_entry<float2>(TN_EINSUM_PASS, out_dev, stream, &bl);
}

// the plan einsum_batched_impl would act on; no GPU needed, none touched
extern "C" int tn_plan_step_batched(int dtype, const u64* out_labels,
                                    const u64* out_shape, size_t out_ndim,
                                    const u64* a_labels, const u64* a_shape,
                                    const i64* a_strides, size_t a_ndim,
                                    const u64* b_labels, const u64* b_shape,
                                    const i64* b_strides, size_t b_ndim,
                                    const u64* batch_labels, size_t nbatch,
                                    int has_stream2, tn_batch_plan* plan) {
  if (!plan || (dtype != 0 && dtype != 1) || out_ndim > TN_MAXR ||
      (nbatch && !batch_labels))
    FAILV(TN_ERR_INVALID,
          "null plan or batch labels, unknown dtype or rank over %d", TN_MAXR);
  Meta A, B;
  int rc = fill_meta(&A, a_labels, a_shape, a_strides, nullptr, a_ndim);
  if (rc) return rc;
  rc = fill_meta(&B, b_labels, b_shape, b_strides, nullptr, b_ndim);
  if (rc) return rc;
  BatchPlan p;
  std::string err;
  rc = plan_step_batched(dtype == 0, out_labels, out_shape, (int)out_ndim, A,
                         B, batch_labels, nbatch, has_stream2 != 0, &p, &err);
  if (rc) {
    g_last_error = err;
    return rc;
  }
  *plan = p;
  return TN_OK;
}

static std::vector<LayoutTensor> layout_leaves(const u64* leaf_labels,
                                               const u64* leaf_dims,
                                               const u64* leaf_nd,
                                               size_t nleaves) {
  std::vector<LayoutTensor> lt(nleaves);
  size_t at = 0;
  for (size_t x = 0; x < nleaves; ++x) {
    lt[x].labels.assign(leaf_labels + at, leaf_labels + at + leaf_nd[x]);
    lt[x].dims.assign(leaf_dims + at, leaf_dims + at + leaf_nd[x]);
    at += leaf_nd[x];
  }
  return lt;
}

extern "C" int tn_plan_batch_walk(int dtype, const u64* leaf_labels,
                                  const u64* leaf_dims, const u64* leaf_nd,
                                  size_t nleaves, const u64* pairs,
                                  size_t nsteps, const u64* batch_labels,
                                  size_t nbatch, int32_t* cls, u64* out_nd,
                                  u64* out_labels, u64* ws_bytes) {
  if ((dtype != 0 && dtype != 1) || (nleaves && !leaf_nd) ||
      (nsteps && !pairs) || (nbatch && !batch_labels))
    FAILV(TN_ERR_INVALID, "unknown dtype or null leaves/pairs/batch labels");
  BatchWalkPlan bw;
  plan_batch_walk(dtype == 0,
                  layout_leaves(leaf_labels, leaf_dims, leaf_nd, nleaves),
                  pairs, nsteps, batch_labels, nbatch, &bw);
  if (!bw.valid) FAILV(TN_ERR_INVALID, "%s", bw.err.c_str());
  for (size_t s = 0; s < nsteps; ++s) {
    if (cls) cls[s] = bw.cls[s];
    if (out_nd) out_nd[s] = bw.out[s].labels.size();
    if (out_labels)
      std::copy(bw.out[s].labels.begin(), bw.out[s].labels.end(),
                out_labels + 64 * s);
    if (ws_bytes) ws_bytes[s] = bw.ws_bytes[s];
  }
  return TN_OK;
}

// --- edge slicing (tn_net_contract_sliced) ---------------------------------
// Both kernels read the assignment from a control record in device memory,
// not from a launch argument: a captured graph of gather -> walk ->
// accumulate is then the same for every assignment.

struct SliceCtl {
  u64 t;      // assignment index, first slice label most significant
  u64 first;  // nonzero: this assignment starts the sum
};

// One sliced leaf: dst[p] = src[base(t) + gather(p)], p over the remaining
// dims (row-major). pstride/dim are shift/mask when pow2 is set, suffix
// product/dim otherwise (the split of k_permute_ct).
struct SliceDesc {
  const void* src;
  void* dst;
  u64 elems;
  int nd, pow2, nsl, pad;
  u64 pstride[TN_MAXR], dim[TN_MAXR], sstride[TN_MAXR];
  // the leaf's slice labels: digit = (t / weight) % radix, times stride
  u64 sl_stride[TN_MAXR], sl_weight[TN_MAXR], sl_radix[TN_MAXR];
};

// blockIdx.y = sliced leaf, grid-stride over its elements in x
template <typename CT>
__global__ void k_slice_gather(const SliceDesc* __restrict__ descs,
                               const SliceCtl* __restrict__ ctl) {
  const SliceDesc& d = descs[blockIdx.y];
  const u64 t = ctl->t;
  u64 base = 0;
  for (int x = 0; x < d.nsl; ++x)
    base += ((t / d.sl_weight[x]) % d.sl_radix[x]) * d.sl_stride[x];
  const CT* __restrict__ src = (const CT*)d.src + base;
  CT* __restrict__ dst = (CT*)d.dst;
  const int nd = d.nd;
  const bool p2 = d.pow2 != 0;
  for (u64 p = blockIdx.x * (u64)blockDim.x + threadIdx.x; p < d.elems;
       p += gridDim.x * (u64)blockDim.x) {
    u64 off = 0;
    for (int i = 0; i < nd; ++i) {
      const u64 c = p2 ? ((p >> d.pstride[i]) & d.dim[i])
                       : ((p / d.pstride[i]) % d.dim[i]);
      off += c * d.sstride[i];
    }
    dst[p] = src[off];
  }
}

// acc[p] = first ? part[p] : acc[p] + part[p], 16 bytes per lane: one c128
// element, or two c64 elements with a scalar tail for an odd count. Plain
// adds in assignment order, so the sum is the IEEE sequence of a host loop
// `total += part`.
__global__ void k_slice_accumulate(double2* __restrict__ acc,
                                   const double2* __restrict__ part, u64 n,
                                   const SliceCtl* __restrict__ ctl) {
  const bool first = ctl->first != 0;
  for (u64 p = blockIdx.x * (u64)blockDim.x + threadIdx.x; p < n;
       p += gridDim.x * (u64)blockDim.x) {
    double2 v = part[p];
    if (!first) {
      const double2 a = acc[p];
      v.x = a.x + v.x;
      v.y = a.y + v.y;
    }
    acc[p] = v;
  }
}

__global__ void k_slice_accumulate(float2* __restrict__ acc,
                                   const float2* __restrict__ part, u64 n,
                                   const SliceCtl* __restrict__ ctl) {
  const bool first = ctl->first != 0;
  const u64 npair = n / 2;
  float4* __restrict__ acc4 = (float4*)acc;
  const float4* __restrict__ part4 = (const float4*)part;
  for (u64 p = blockIdx.x * (u64)blockDim.x + threadIdx.x; p < npair;
       p += gridDim.x * (u64)blockDim.x) {
    float4 v = part4[p];
    if (!first) {
      const float4 a = acc4[p];
      v.x = a.x + v.x;
      v.y = a.y + v.y;
      v.z = a.z + v.z;
      v.w = a.w + v.w;
    }
    acc4[p] = v;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    float2 v = part[n - 1];
    if (!first) {
      const float2 a = acc[n - 1];
      v.x = a.x + v.x;
      v.y = a.y + v.y;
    }
    acc[n - 1] = v;
  }
}

// ---------------------------------------------------------------------------
// network executor (contract_tensor_network replacement)
// ---------------------------------------------------------------------------

// labels and dims in stored order, contiguous row-major on the device
struct DevTensor : LayoutTensor {
  void* data = nullptr;
  u64 elems = 1;
  bool owned = false;     // intermediate owned by the walk (freed on consume)
  bool external = false;  // caller-owned device buffer (never freed by us)
};

// What tn_net_contract_sliced keeps per (path, slice labels): the slice plan
// with its reduced walk plan, the shadow leaves (one slab, rewritten by
// k_slice_gather for every assignment), the descriptor table and the control
// record on the device, and the captured graph of one assignment.
struct SliceState {
  std::vector<u64> pairs, labels;  // the key
  SlicePlan plan;
  std::vector<DevTensor> leaves;  // shadows where sliced, originals otherwise
  void* slab = nullptr;           // the shadow leaves' storage
  bool slab_in_arena = false;
  void* descs = nullptr;  // SliceDesc[ndesc]
  unsigned ndesc = 0;
  u64 max_elems = 0;      // largest shadow leaf
  void* ctl = nullptr;    // SliceCtl the kernels read
  void* table = nullptr;  // SliceCtl[table_cap], one per listed assignment
  size_t table_cap = 0;
  // graph of gather -> walk -> accumulate; states as tn_net::graph_state
  hipGraphExec_t graph_exec = nullptr;
  int graph_state = 0;
  void* graph_acc = nullptr;  // the accumulator address the graph bakes

  void drop_graph() {
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    graph_exec = nullptr;
    graph_acc = nullptr;
    if (graph_state > 0) graph_state = 0;
  }
};

struct tn_net {
  int device = 0;
  int dtype = 0;   // 0 = c128, 1 = c64
  size_t esize = 16;
  hipStream_t stream = nullptr;
  hipStream_t stream2 = nullptr;  // pack-overlap stream (prepack permutes)
  std::vector<DevTensor> leaves;
  DevTensor final_t;       // final tensor of the last contract (owned)
  bool final_in_arena = false;
  bool has_final = false;
  Arena arena;
  u64 pool_in_use = 0;
  // hipGraph replay of the (launch-bound) walk: captured after the first
  // normal run when every workspace block came from the arena, so the
  // graph's baked device pointers are stable across replays (the arena's
  // host-side first-fit is deterministic and the final block stays
  // reserved). Invalidated by a different path or new leaves.
  hipGraphExec_t graph_exec = nullptr;
  std::vector<u64> graph_pairs;
  // the walk plan (plan_layouts): stored out order and look-ahead pack of
  // every step, kept per path
  LayoutPlan layout;
  std::vector<u64> layout_pairs;
  bool layout_known = false;
  int graph_state = 0;  // 0 = no normal run yet, 1 = ready to capture,
                        // 2 = captured, -1 = disabled (spill/failure)

  // edge slicing: the state of the last (path, slice labels) contracted. Its
  // graph and the one above never coexist: a sliced call drops the unsliced
  // graph and an unsliced call the sliced one, since each walk's arena
  // blocks are free for the other to take.
  SliceState* slices = nullptr;

  // tn_net_contract_batched under a captured graph: the graph bakes the
  // address of its final tensor, so that block stays reserved here while
  // final_t holds the batched result; the next plain call takes it back
  // (restore_graph_final) before it replays. Always an arena block.
  DevTensor graph_final;

  void drop_graph() {
    if (graph_final.data) arena.release(graph_final.data);
    graph_final = DevTensor();
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    graph_exec = nullptr;
    graph_pairs.clear();
    if (graph_state > 0) graph_state = 0;
  }

  void drop_slices() {
    if (!slices) return;
    (void)hipStreamSynchronize(stream);
    slices->drop_graph();
    if (slices->slab) {
      if (slices->slab_in_arena)
        arena.release(slices->slab);
      else
        (void)hipFree(slices->slab);
    }
    if (slices->descs) (void)hipFree(slices->descs);
    if (slices->ctl) (void)hipFree(slices->ctl);
    if (slices->table) (void)hipFree(slices->table);
    delete slices;
    slices = nullptr;
  }

  void invalidate_graph() {
    drop_graph();
    layout_known = false;  // same triggers: the network or the arena changed
    drop_slices();
  }
};

extern "C" tn_net* tn_net_create2(int device, int dtype) {
  if (dtype != 0 && dtype != 1) {
    g_last_error = "dtype must be 0 (c128) or 1 (c64)";
    return nullptr;
  }
  if (tn_device_count() == 0) {
    g_last_error = "no AMD GPU present — tnc_hip has no CPU fallback by design";
    return nullptr;
  }
  if (hipSetDevice(device) != hipSuccess) {
    g_last_error = "hipSetDevice failed";
    return nullptr;
  }
  ensure_mempool(device);
  tn_net* net = new tn_net();
  net->device = device;
  net->dtype = dtype;
  net->esize = dtype == 0 ? 16 : 8;
  if (hipStreamCreate(&net->stream) != hipSuccess) {
    delete net;
    g_last_error = "hipStreamCreate failed";
    return nullptr;
  }
  if (hipStreamCreate(&net->stream2) != hipSuccess) {
    (void)hipStreamDestroy(net->stream);
    delete net;
    g_last_error = "hipStreamCreate failed";
    return nullptr;
  }
  return net;
}

extern "C" tn_net* tn_net_create(int device) {
  return tn_net_create2(device, 0);
}

extern "C" int tn_net_reserve(tn_net* net, uint64_t bytes) {
  if (!net) FAILV(TN_ERR_INVALID, "null net");
  net->invalidate_graph();
  HIP_CHECK(hipSetDevice(net->device));
  if (net->arena.reserve(bytes))
    FAILV(TN_ERR_OOM, "arena reservation of %llu bytes failed",
          (unsigned long long)bytes);
  return TN_OK;
}

extern "C" int64_t tn_net_add_leaf(tn_net* net, const u64* labels,
                                   const u64* dims, size_t ndim,
                                   const void* host_data) {
  if (!net) return -TN_ERR_INVALID;
  if (ndim > TN_MAXR) {
    g_last_error = "rank too large";
    return -TN_ERR_INVALID;
  }
  net->invalidate_graph();  // the network changed
  if (hipSetDevice(net->device) != hipSuccess) return -TN_ERR_HIP;
  DevTensor t;
  t.labels.assign(labels, labels + ndim);
  t.dims.assign(dims, dims + ndim);
  for (size_t i = 0; i < ndim; ++i) t.elems *= dims[i];
  if (hipMalloc((void**)&t.data, t.elems * net->esize) != hipSuccess) {
    g_last_error = "hipMalloc failed for leaf";
    return -TN_ERR_OOM;
  }
  if (hipMemcpy(t.data, host_data, t.elems * net->esize,
                hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(t.data);
    g_last_error = "hipMemcpy failed for leaf";
    return -TN_ERR_HIP;
  }
  t.owned = false;  // leaves persist; freed only at destroy
  net->leaves.push_back(std::move(t));
  return (int64_t)net->leaves.size() - 1;
}

extern "C" int64_t tn_net_add_leaf_dev(tn_net* net, const u64* labels,
                                       const u64* dims, size_t ndim,
                                       void* dev_data) {
  if (!net) return -TN_ERR_INVALID;
  if (ndim > TN_MAXR) {
    g_last_error = "rank too large";
    return -TN_ERR_INVALID;
  }
  net->invalidate_graph();  // the network changed
  DevTensor t;
  t.labels.assign(labels, labels + ndim);
  t.dims.assign(dims, dims + ndim);
  for (size_t i = 0; i < ndim; ++i) t.elems *= dims[i];
  t.data = dev_data;
  t.owned = false;
  t.external = true;
  net->leaves.push_back(std::move(t));
  return (int64_t)net->leaves.size() - 1;
}

// release the previous final tensor. Never inside a stream capture: the
// release may hipFree, and hipFree device-syncs.
static void release_final(tn_net* net) {
  if (!net->has_final || !net->final_t.owned) return;
  if (net->final_in_arena)
    net->arena.release(net->final_t.data);
  else
    (void)hipFree(net->final_t.data);
  net->final_t = DevTensor();
  net->has_final = false;
  net->final_in_arena = false;
}

// the walk plan of this path over the net's leaves, computed once per path
static const LayoutPlan& walk_plan(tn_net* net, const u64* pairs,
                                   size_t nsteps) {
  if (!net->layout_known || net->layout_pairs.size() != 2 * nsteps ||
      !std::equal(net->layout_pairs.begin(), net->layout_pairs.end(), pairs)) {
    const std::vector<LayoutTensor> lt(net->leaves.begin(), net->leaves.end());
    plan_layouts(net->dtype == 0, lt, pairs, nsteps, &net->layout);
    net->layout_pairs.assign(pairs, pairs + 2 * nsteps);
    net->layout_known = true;
  }
  return net->layout;
}

// the one place the walk switches on dtype: f gets a null CT* as a type tag
template <typename F>
static int with_dtype(int dtype, F&& f) {
  return dtype == 0 ? f((double2*)nullptr) : f((float2*)nullptr);
}

// per-step outputs of a profiled walk (step_ms null: a plain walk)
struct StepTimes {
  double* step_ms = nullptr;
  double* gemm_ms = nullptr;
  int32_t* kind = nullptr;
};

// what a walk under stream capture leaves for after EndCapture
struct CaptureLog {
  std::vector<void*> deferred;  // non-arena blocks to hipFree
  bool spilled = false;         // a block came from outside the arena
};

// One contraction's transient state. The destructor gives back whatever the
// walk still holds, so every exit from contract_impl and from the pieces
// below is a plain return.
//
// Pack overlap: while step s runs on net->stream, the NEXT step's GEMM pack
// permutes run on net->stream2 (after an event marking steps < s complete).
// A prepacked slot becomes a contiguous tensor in pack order, which the step
// then finds ready; an operand not prepacked is packed inline. The replaced
// originals are freed at the top of step s+1, after the main stream waits on
// the packs — so every arena block's next user is ordered behind its last
// reader, preserving the arena's stream-ordered reuse contract across both
// streams.
struct Walk {
  tn_net* const net;
  CaptureLog* const cap;  // null: a normal run
  WsCtx ws;
  std::vector<DevTensor> slots;  // the leaves (not owned), then intermediates
  std::vector<char> alive;
  DevTensor out;                 // the current step's output, until retired
  std::vector<void*> pending;    // owned originals a prepack replaced
  hipEvent_t pending_done = nullptr;  // the packs of `pending` have run
  // every event of the walk, the pack pipeline's included (ws.events);
  // destroyed when the walk is over
  std::vector<hipEvent_t> events;
  std::vector<hipEvent_t> prof_ev;  // per step: start, end, gemm start, end
  hipEvent_t walk_start = nullptr, walk_end = nullptr;
  const bool overlap;
  // false: one assignment of a sliced run, which neither synchronises nor
  // times itself (tn_net_contract_sliced times the whole call)
  const bool timed;
  bool done = false;  // the final tensor was handed over
  // tn_net_contract_batched: dispatch goes to einsum_batched_impl
  bool batched = false;
  const u64* batch_labels = nullptr;
  size_t nbatch = 0;

  // `leaves`: the net's own, or a sliced run's shadow leaves in their place
  Walk(tn_net* n, CaptureLog* c, const std::vector<DevTensor>& leaves,
       bool timed_ = true)
      : net(n), cap(c),
        ws{n->arena.base ? &n->arena : nullptr, n->stream, c != nullptr, false,
           c ? &c->deferred : nullptr},
        slots(leaves), alive(leaves.size(), 1),
        overlap(!env_switch(ENV_NO_PREPACK) && n->stream2 &&
                n->arena.base != nullptr),
        timed(timed_) {
    ws.stream2 = n->stream2;
    ws.events = &events;
    for (auto& s : slots) s.owned = false;  // shallow copies
  }
  Walk(const Walk&) = delete;

  ~Walk() {
    if (!done && !cap) {
      (void)hipStreamSynchronize(net->stream);
      (void)hipStreamSynchronize(net->stream2);
    }
    // left by an early exit: deferred originals, the current out, owned
    // intermediates
    for (void* p : pending) ws_free(ws, p);
    if (out.owned) ws_free(ws, out.data);
    for (size_t x = 0; x < slots.size(); ++x)
      if (alive[x] && slots[x].owned) ws_free(ws, slots[x].data);
    for (hipEvent_t e : events) (void)hipEventDestroy(e);
    if (cap) cap->spilled = ws.spilled;
  }

  hipEvent_t new_event() {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    events.push_back(e);
    return e;
  }

  int begin(size_t nsteps, bool profiled) {
    for (size_t x = 0; profiled && x < 4 * nsteps; ++x) {
      prof_ev.push_back(new_event());
      if (!prof_ev.back()) FAILV(TN_ERR_HIP, "hipEventCreate failed");
    }
    if (cap || !timed) return TN_OK;
    HIP_CHECK(hipStreamSynchronize(net->stream));
    walk_start = new_event();
    walk_end = new_event();
    if (!walk_start || !walk_end) FAILV(TN_ERR_HIP, "hipEventCreate failed");
    HIP_CHECK(hipEventRecord(walk_start, net->stream));
    return TN_OK;
  }

  // join this step's prepack (issued during the step before): free the
  // replaced originals only now, behind the wait, so their blocks cannot be
  // re-handed while the pack kernels still read them
  int join_prepack() {
    if (!pending_done) return TN_OK;
    if (hipStreamWaitEvent(net->stream, pending_done, 0) != hipSuccess)
      FAILV(TN_ERR_HIP, "hipStreamWaitEvent failed (prepack join)");
    for (void* p : pending) ws_free(ws, p);
    pending.clear();
    pending_done = nullptr;
    return TN_OK;
  }

  int alloc_out(const LayoutTensor& order) {
    out = DevTensor();
    out.labels = order.labels;
    out.dims = order.dims;
    for (u64 d : out.dims) out.elems *= d;
    if (ws_alloc(ws, &out.data, out.elems * net->esize) != TN_OK) {
      out.data = nullptr;
      FAILV(TN_ERR_OOM, "device allocation failed for intermediate");
    }
    out.owned = true;
    return TN_OK;
  }

  // pack slot S into *dst in the given axis order on stream2; S adopts *dst
  int pack_slot(DevTensor& S, const std::vector<int>& axes, u64 elems,
                void** dst) {
    Meta ms;
    layout_meta(S, &ms, S.data);
    std::vector<AxisInfo> ax;
    LayoutTensor packed;
    for (int axis : axes) {
      ax.push_back({ms.dims[axis], ms.strides[axis], 0});
      packed.labels.push_back(S.labels[axis]);
      packed.dims.push_back(S.dims[axis]);
    }
    int rc = with_dtype(net->dtype, [&](auto* t) {
      typedef std::remove_pointer_t<decltype(t)> CT;
      return launch_permute((const CT*)S.data, (CT*)*dst, elems, ax,
                            net->stream2);
    });
    if (rc != TN_OK) return rc;
    if (S.owned) pending.push_back(S.data);
    static_cast<LayoutTensor&>(S) = std::move(packed);
    S.data = *dst;
    S.owned = true;
    S.external = false;
    *dst = nullptr;
    return TN_OK;
  }

  // the two events, then the packs on stream2 behind all the main stream
  // has been given so far; without events the step packs inline
  int launch_prepack(const EarlyPack& e, u64 ni, u64 nj, void* dst[2]) {
    hipEvent_t ready = new_event();
    hipEvent_t packed = ready ? new_event() : nullptr;
    if (!packed) return TN_OK;
    if (hipEventRecord(ready, net->stream) != hipSuccess ||
        hipStreamWaitEvent(net->stream2, ready, 0) != hipSuccess)
      FAILV(TN_ERR_HIP, "prepack event sync failed");
    int rc = TN_OK;
    if (e.a) rc = pack_slot(slots[ni], e.a_axes, e.a_elems, &dst[0]);
    if (rc == TN_OK && e.b)
      rc = pack_slot(slots[nj], e.b_axes, e.b_elems, &dst[1]);
    if (rc != TN_OK) return rc;
    if (hipEventRecord(packed, net->stream2) != hipSuccess)
      FAILV(TN_ERR_HIP, "prepack event record failed");
    pending_done = packed;
    return TN_OK;
  }

  // Act on the planned look-ahead pack of the next step (operands ni, nj),
  // overlapping this step's kernels. Arena only, both buffers or none; on
  // any shortage the step simply packs inline.
  int issue_prepack(const EarlyPack& e, u64 ni, u64 nj) {
    if (!overlap || !(e.a || e.b)) return TN_OK;
    Arena& arena = net->arena;
    void* dst[2] = {e.a ? arena.alloc(e.a_elems * net->esize) : nullptr,
                    e.b ? arena.alloc(e.b_elems * net->esize) : nullptr};
    int rc = TN_OK;
    if ((!e.a || dst[0]) && (!e.b || dst[1]))
      rc = launch_prepack(e, ni, nj, dst);
    for (void* p : dst)  // not adopted by a slot: a shortage, or a failure
      if (p) arena.release(p);
    return rc;
  }

  // Plan and run step s on the operands as they sit on the device now
  // (einsum_dev_impl: a failed prepack, or a prepacked A that turns the pack
  // pipeline off, is its business).
  int dispatch(size_t s, const DevTensor& A, const DevTensor& B,
               const StepTimes& times) {
    const bool profiled = !prof_ev.empty();
    Meta ma, mb;
    layout_meta(A, &ma, A.data);
    layout_meta(B, &mb, B.data);
    StepStats st{};
    if (profiled) {
      HIP_CHECK(hipEventRecord(prof_ev[4 * s], net->stream));
      st.gemm_ev0 = prof_ev[4 * s + 2];
      st.gemm_ev1 = prof_ev[4 * s + 3];
    }
    int rc = with_dtype(net->dtype, [&](auto* t) {
      typedef std::remove_pointer_t<decltype(t)> CT;
      if (batched)
        return einsum_batched_impl<CT>(
            out.labels.data(), out.dims.data(), (int)out.labels.size(), ma, mb,
            batch_labels, nbatch, (CT*)out.data, net->stream, ws, &st);
      return einsum_dev_impl<CT>(out.labels.data(), out.dims.data(),
                                 (int)out.labels.size(), ma, mb, (CT*)out.data,
                                 net->stream, ws, &st);
    });
    if (profiled) HIP_CHECK(hipEventRecord(prof_ev[4 * s + 1], net->stream));
    if (times.kind) times.kind[s] = st.kind;
    // only TTGT steps (kind 2/3) record the gemm events; probing unrecorded
    // events would fail AND leave a sticky TLS error
    if (profiled && st.kind != 2 && st.kind != 3) prof_ev[4 * s + 2] = nullptr;
    if (rc != TN_OK) {
      char buf[96];
      snprintf(buf, sizeof buf, " (at step %zu, out elems %llu)", s,
               (unsigned long long)out.elems);
      g_last_error += buf;
    }
    return rc;
  }

  // free consumed intermediates (leaves persist); out takes A's slot
  void retire(u64 i, u64 j) {
    if (slots[i].owned) ws_free(ws, slots[i].data);
    if (slots[j].owned) ws_free(ws, slots[j].data);
    slots[i] = std::move(out);
    out = DevTensor();
    alive[j] = 0;
  }

  // close the timed span and read the timings back
  int read_times(size_t nsteps, const StepTimes& times, double* elapsed_ms) {
    float ms = 0.f;
    if (!cap && timed) {
      HIP_CHECK(hipEventRecord(walk_end, net->stream));
      HIP_CHECK(hipStreamSynchronize(net->stream));
      HIP_CHECK(hipEventElapsedTime(&ms, walk_start, walk_end));
    }
    if (elapsed_ms) *elapsed_ms = (double)ms;
    if (prof_ev.empty()) return TN_OK;
    for (size_t s = 0; s < nsteps; ++s) {
      float sms = 0.f, gms = 0.f;
      HIP_CHECK(hipEventElapsedTime(&sms, prof_ev[4 * s], prof_ev[4 * s + 1]));
      times.step_ms[s] = (double)sms;
      if (prof_ev[4 * s + 2] &&
          hipEventElapsedTime(&gms, prof_ev[4 * s + 2], prof_ev[4 * s + 3]) !=
              hipSuccess)
        gms = 0.f;
      if (times.gemm_ms) times.gemm_ms[s] = (double)gms;
    }
    (void)hipGetLastError();  // clear any error from unrecorded-event reads
    return TN_OK;
  }

  // the one tensor left becomes the net's final tensor
  int hand_over() {
    size_t x = 0;
    while (!alive[x]) ++x;
    DevTensor& f = slots[x];
    if (f.owned) {
      net->final_in_arena = ws.arena && ws.arena->owns(f.data);
      net->final_t = std::move(f);
      f.owned = false;
    } else {
      // final == a leaf (empty path): copy so result is stable
      DevTensor c = f;
      if (hipMalloc(&c.data, f.elems * net->esize) != hipSuccess)
        FAILV(TN_ERR_OOM, "hipMalloc failed for final copy");
      if (hipMemcpy(c.data, f.data, f.elems * net->esize,
                    hipMemcpyDeviceToDevice) != hipSuccess) {
        (void)hipFree(c.data);
        FAILV(TN_ERR_HIP, "hipMemcpy failed for final copy");
      }
      c.owned = true;
      net->final_t = std::move(c);
    }
    net->has_final = true;
    done = true;
    return TN_OK;
  }

  // a sliced run's ending: the one tensor left is this assignment's part of
  // the sum. Add it to acc (or start acc with it) and give its block back;
  // the next user of the block is ordered behind the kernel on the stream.
  int fold_into(void* acc, const void* ctl) {
    size_t x = 0;
    while (!alive[x]) ++x;
    DevTensor& f = slots[x];
    with_dtype(net->dtype, [&](auto* t) {
      typedef std::remove_pointer_t<decltype(t)> CT;
      const u64 lanes = sizeof(CT) == 16 ? f.elems : (f.elems + 1) / 2;
      k_slice_accumulate<<<grid_for(lanes), 256, 0, net->stream>>>(
          (CT*)acc, (const CT*)f.data, f.elems, (const SliceCtl*)ctl);
      return 0;
    });
    HIP_CHECK(hipGetLastError());
    if (f.owned) ws_free(ws, f.data);
    f.owned = false;
    done = true;
    return TN_OK;
  }
};

// the step loop of a walk: join, allocate, look ahead, dispatch, retire
static int walk_steps(Walk& w, const LayoutPlan& plan, const u64* pairs,
                      size_t nsteps, const StepTimes& times) {
  for (size_t s = 0; s < nsteps; ++s) {
    const u64 i = pairs[2 * s], j = pairs[2 * s + 1];
    int rc = w.join_prepack();
    if (rc == TN_OK) rc = w.alloc_out(plan.out[s]);
    if (rc == TN_OK && s + 1 < nsteps)
      rc = w.issue_prepack(plan.early[s + 1], pairs[2 * s + 2],
                           pairs[2 * s + 3]);
    if (rc == TN_OK) rc = w.dispatch(s, w.slots[i], w.slots[j], times);
    if (rc != TN_OK) return rc;
    w.retire(i, j);
  }
  return TN_OK;
}

static int contract_impl(tn_net* net, const u64* pairs, size_t nsteps,
                         const StepTimes& times, double* elapsed_ms,
                         CaptureLog* cap = nullptr) {
  if (!net) FAILV(TN_ERR_INVALID, "null net");
  HIP_CHECK(hipSetDevice(net->device));
  release_final(net);
  const LayoutPlan& plan = walk_plan(net, pairs, nsteps);
  if (!plan.valid) FAILV(TN_ERR_INVALID, "%s", plan.err.c_str());
  if (net->leaves.size() != nsteps + 1)
    FAILV(TN_ERR_INVALID, "path did not fully contract the network");
  Walk w(net, cap, net->leaves);
  if (int rc = w.begin(nsteps, times.step_ms != nullptr)) return rc;
  if (int rc = walk_steps(w, plan, pairs, nsteps, times)) return rc;
  if (int rc = w.read_times(nsteps, times, elapsed_ms)) return rc;
  return w.hand_over();
}

static bool graph_pairs_match(const tn_net* net, const u64* pairs,
                              size_t nsteps) {
  return net->graph_pairs.size() == 2 * nsteps &&
         std::equal(net->graph_pairs.begin(), net->graph_pairs.end(), pairs);
}

static int contract_graph_replay(tn_net* net, double* elapsed_ms) {
  HIP_CHECK(hipSetDevice(net->device));
  hipEvent_t e0 = nullptr, e1 = nullptr;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));
  HIP_CHECK(hipEventRecord(e0, net->stream));
  if (hipGraphLaunch(net->graph_exec, net->stream) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    net->invalidate_graph();
    net->graph_state = -1;
    FAILV(TN_ERR_HIP, "hipGraphLaunch failed");
  }
  HIP_CHECK(hipEventRecord(e1, net->stream));
  HIP_CHECK(hipStreamSynchronize(net->stream));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (elapsed_ms) *elapsed_ms = (double)ms;
  // bookkeeping is untouched: the replay rewrites the same arena blocks and
  // the final tensor lands at its captured address (net->final_t)
  net->has_final = true;
  return TN_OK;
}

static int contract_graph_capture(tn_net* net, const u64* pairs,
                                  size_t nsteps) {
  HIP_CHECK(hipSetDevice(net->device));
  release_final(net);  // outside the capture; the walk then finds none
  HIP_CHECK(hipStreamSynchronize(net->stream));
  if (hipStreamBeginCapture(net->stream, hipStreamCaptureModeThreadLocal) !=
      hipSuccess) {
    (void)hipGetLastError();
    net->graph_state = -1;
    return TN_ERR_HIP;
  }
  CaptureLog cap;
  int rc = contract_impl(net, pairs, nsteps, StepTimes(), nullptr, &cap);
  hipGraph_t g = nullptr;
  hipError_t ce = hipStreamEndCapture(net->stream, &g);
  for (void* p : cap.deferred) (void)hipFree(p);
  (void)hipGetLastError();
  if (rc != TN_OK || ce != hipSuccess || !g || cap.spilled) {
    if (g) (void)hipGraphDestroy(g);
    net->graph_state = -1;  // caller falls back to a normal run
    return rc != TN_OK ? rc : TN_ERR_HIP;
  }
  hipGraphExec_t exec = nullptr;
  if (hipGraphInstantiate(&exec, g, nullptr, nullptr, 0) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipGraphDestroy(g);
    net->graph_state = -1;
    return TN_ERR_HIP;
  }
  (void)hipGraphDestroy(g);
  net->graph_exec = exec;
  net->graph_state = 2;
  return TN_OK;
}

// after tn_net_contract_batched: the captured graph's final block becomes
// the net's final tensor again, as the replay expects to find it
static void restore_graph_final(tn_net* net) {
  if (!net->graph_final.data) return;
  release_final(net);  // the batched result
  net->final_t = std::move(net->graph_final);
  net->graph_final = DevTensor();
  net->final_in_arena = true;
  net->has_final = true;
}

extern "C" int tn_net_contract_batched(tn_net* net, const u64* pairs,
                                       size_t nsteps, const u64* batch_labels,
                                       size_t nbatch, double* elapsed_ms) {
  if (!net) FAILV(TN_ERR_INVALID, "null net");
  if ((nsteps && !pairs) || (nbatch && !batch_labels))
    FAILV(TN_ERR_INVALID, "null pairs or batch labels");
  if (net->leaves.size() != nsteps + 1)
    FAILV(TN_ERR_INVALID, "path did not fully contract the network");
  HIP_CHECK(hipSetDevice(net->device));
  BatchWalkPlan bw;
  plan_batch_walk(
      net->dtype == 0,
      std::vector<LayoutTensor>(net->leaves.begin(), net->leaves.end()), pairs,
      nsteps, batch_labels, nbatch, &bw);
  if (!bw.valid) FAILV(TN_ERR_INVALID, "%s", bw.err.c_str());
  if (net->slices) net->slices->drop_graph();  // its blocks are ours to take
  // The plain walk's cached plan and captured graph stay. The graph's final
  // block is set aside, reserved, so this walk's result lands elsewhere.
  if (net->graph_state == 2 && !net->graph_final.data && net->has_final &&
      net->final_t.owned && net->final_in_arena) {
    net->graph_final = std::move(net->final_t);
    net->final_t = DevTensor();
    net->has_final = false;
    net->final_in_arena = false;
  } else {
    release_final(net);
  }
  Walk w(net, nullptr, net->leaves);
  w.batched = true;
  w.batch_labels = batch_labels;
  w.nbatch = nbatch;
  if (int rc = w.begin(nsteps, false)) return rc;
  for (size_t s = 0; s < nsteps; ++s) {
    const u64 i = pairs[2 * s], j = pairs[2 * s + 1];
    if (int rc = w.alloc_out(bw.out[s])) return rc;
    if (int rc = w.dispatch(s, w.slots[i], w.slots[j], StepTimes()))
      return rc;
    w.retire(i, j);
  }
  if (int rc = w.read_times(nsteps, StepTimes(), elapsed_ms)) return rc;
  return w.hand_over();
}

extern "C" int tn_net_contract(tn_net* net, const u64* pairs, size_t nsteps,
                               double* elapsed_ms) {
  if (!net) FAILV(TN_ERR_INVALID, "null net");
  restore_graph_final(net);
  if (net->slices) net->slices->drop_graph();  // its blocks are ours to take
  if (net->graph_state == 2) {
    // a failed walk since capture clears final_t, whose address the replay
    // relies on — in that case re-run (and re-capture) normally
    if (graph_pairs_match(net, pairs, nsteps) && net->final_t.data)
      return contract_graph_replay(net, elapsed_ms);
    net->invalidate_graph();  // different path / lost state: re-arm below
  }
  if (net->graph_state == 1 && net->arena.base &&
      graph_pairs_match(net, pairs, nsteps)) {
    if (contract_graph_capture(net, pairs, nsteps) == TN_OK)
      return contract_graph_replay(net, elapsed_ms);
    // capture failed (workspace spill etc.) — run normally below
  }
  int rc = contract_impl(net, pairs, nsteps, StepTimes(), elapsed_ms);
  if (rc == TN_OK && net->graph_state >= 0 && net->arena.base) {
    net->graph_pairs.assign(pairs, pairs + 2 * nsteps);
    net->graph_state = 1;  // arm capture for the next identical call
  }
  return rc;
}

extern "C" int tn_net_contract_profiled(tn_net* net, const u64* pairs,
                                        size_t nsteps, double* step_ms,
                                        double* gemm_ms, int32_t* kind,
                                        double* elapsed_ms) {
  if (!net) FAILV(TN_ERR_INVALID, "null net");
  restore_graph_final(net);
  if (net->slices) net->slices->drop_graph();
  if (net->graph_state == 2 && !graph_pairs_match(net, pairs, nsteps))
    net->invalidate_graph();  // different path moves the final block
  int rc = contract_impl(net, pairs, nsteps, StepTimes{step_ms, gemm_ms, kind},
                         elapsed_ms);
  if (rc == TN_OK && net->graph_state == 0 && net->arena.base) {
    net->graph_pairs.assign(pairs, pairs + 2 * nsteps);
    net->graph_state = 1;  // a profiled pass also arms graph capture
  }
  return rc;
}

// ---- sliced contraction ---------------------------------------------------
// The sum over slice assignments of the network with the slice labels fixed:
// per assignment one gather of the sliced leaves into their shadows, the
// same walk over the reduced plan, and one accumulate of its final tensor.
// The assignment reaches the kernels through the control record, which a
// 16-byte device-to-device copy sets between walks, so the host never waits
// between assignments and one captured graph serves them all.

// shadow leaves, descriptor table and control record of a fresh slice plan
static int build_slice_buffers(tn_net* net, SliceState& S) {
  const SlicePlan& sp = S.plan;
  const size_t n = net->leaves.size(), nl = sp.labels.size();
  S.leaves.assign(net->leaves.begin(), net->leaves.end());
  std::vector<u64> off(n, 0);
  u64 total = 0;
  for (size_t x = 0; x < n; ++x) {
    S.leaves[x].owned = false;
    if (!sp.sliced[x]) continue;
    u64 elems = 1;
    for (u64 d : sp.reduced[x].dims) elems *= d;
    off[x] = total;
    total += (elems * net->esize + 255) & ~(u64)255;
    S.max_elems = std::max(S.max_elems, elems);
    ++S.ndesc;
  }
  if (S.ndesc > 65535) FAILV(TN_ERR_INVALID, "more than 65535 sliced leaves");
  if (total) {
    S.slab = net->arena.alloc(total);
    S.slab_in_arena = S.slab != nullptr;
    if (!S.slab && hipMalloc(&S.slab, total) != hipSuccess) {
      (void)hipGetLastError();
      S.slab = nullptr;
      FAILV(TN_ERR_OOM, "device allocation failed for the shadow leaves");
    }
  }
  std::vector<SliceDesc> descs;
  for (size_t x = 0; x < n; ++x) {
    if (!sp.sliced[x]) continue;
    const DevTensor& full = net->leaves[x];
    DevTensor& sh = S.leaves[x];
    static_cast<LayoutTensor&>(sh) = sp.reduced[x];
    sh.elems = 1;
    for (u64 d : sh.dims) sh.elems *= d;
    sh.data = (char*)S.slab + off[x];
    sh.external = true;  // the slab is the state's, never a walk's
    SliceDesc d{};
    d.src = full.data;
    d.dst = sh.data;
    d.elems = sh.elems;
    // remaining axes of the stored leaf, with their source strides
    std::vector<AxisInfo> ax;
    u64 stride = 1;
    for (size_t a = full.labels.size(); a-- > 0;) {
      if (std::find(sp.labels.begin(), sp.labels.end(), full.labels[a]) ==
          sp.labels.end())
        ax.insert(ax.begin(), AxisInfo{full.dims[a], (i64)stride, 0});
      stride *= full.dims[a];
    }
    d.nd = (int)ax.size();
    d.pow2 = axes_pow2(ax) ? 1 : 0;
    u64 pstride = 1;
    for (int i = d.nd - 1; i >= 0; --i) {
      d.pstride[i] = d.pow2 ? (u64)log2_u64(pstride) : pstride;
      d.dim[i] = d.pow2 ? ax[i].dim - 1 : ax[i].dim;
      d.sstride[i] = (u64)ax[i].sa;
      pstride *= ax[i].dim;
    }
    for (size_t l = 0; l < nl; ++l) {
      if (!sp.strides[x * nl + l]) continue;
      d.sl_stride[d.nsl] = sp.strides[x * nl + l];
      d.sl_weight[d.nsl] = sp.weights[l];
      d.sl_radix[d.nsl] = sp.radices[l];
      ++d.nsl;
    }
    descs.push_back(d);
  }
  if (!descs.empty()) {
    HIP_CHECK(hipMalloc(&S.descs, descs.size() * sizeof(SliceDesc)));
    HIP_CHECK(hipMemcpy(S.descs, descs.data(),
                        descs.size() * sizeof(SliceDesc),
                        hipMemcpyHostToDevice));
  }
  HIP_CHECK(hipMalloc(&S.ctl, sizeof(SliceCtl)));
  return TN_OK;
}

// the net's slice state for this (path, slice labels), built when the key
// differs. A refused plan leaves the net as it was.
static int slice_state(tn_net* net, const u64* pairs, size_t nsteps,
                       const u64* labels, size_t nlabels, SliceState** out) {
  SliceState* S = net->slices;
  if (S && S->pairs.size() == 2 * nsteps && S->labels.size() == nlabels &&
      std::equal(S->pairs.begin(), S->pairs.end(), pairs) &&
      std::equal(S->labels.begin(), S->labels.end(), labels)) {
    *out = S;
    return TN_OK;
  }
  S = new SliceState();
  const std::vector<LayoutTensor> lt(net->leaves.begin(), net->leaves.end());
  plan_slices(net->dtype == 0, lt, pairs, nsteps, labels, nlabels, &S->plan);
  if (!S->plan.valid) {
    g_last_error = S->plan.err;
    delete S;
    return TN_ERR_INVALID;
  }
  net->drop_slices();
  S->pairs.assign(pairs, pairs + 2 * nsteps);
  S->labels.assign(labels, labels + nlabels);
  net->slices = S;
  if (int rc = build_slice_buffers(net, *S)) {
    const std::string why = g_last_error;
    net->drop_slices();
    g_last_error = why;
    return rc;
  }
  *out = S;
  return TN_OK;
}

// one assignment: gather -> walk -> accumulate, on net->stream
static int sliced_unit(tn_net* net, SliceState& S, void* acc,
                       CaptureLog* cap) {
  const size_t nsteps = S.pairs.size() / 2;
  if (S.ndesc) {
    const dim3 grid((unsigned)grid_for(S.max_elems), S.ndesc);
    with_dtype(net->dtype, [&](auto* t) {
      typedef std::remove_pointer_t<decltype(t)> CT;
      k_slice_gather<CT><<<grid, 256, 0, net->stream>>>(
          (const SliceDesc*)S.descs, (const SliceCtl*)S.ctl);
      return 0;
    });
    HIP_CHECK(hipGetLastError());
  }
  Walk w(net, cap, S.leaves, false);
  if (int rc = w.begin(nsteps, false)) return rc;
  if (int rc = walk_steps(w, S.plan.layout, S.pairs.data(), nsteps,
                          StepTimes()))
    return rc;
  return w.fold_into(acc, S.ctl);
}

// capture one assignment's unit; on any failure the state is -1 and the
// caller runs the assignment normally (nothing of the capture has executed)
static int sliced_capture(tn_net* net, SliceState& S, void* acc) {
  // the one host wait besides the call's last: when the graph is (re)built
  HIP_CHECK(hipStreamSynchronize(net->stream));
  if (hipStreamBeginCapture(net->stream, hipStreamCaptureModeThreadLocal) !=
      hipSuccess) {
    (void)hipGetLastError();
    S.graph_state = -1;
    return TN_ERR_HIP;
  }
  CaptureLog cap;
  int rc = sliced_unit(net, S, acc, &cap);
  hipGraph_t g = nullptr;
  hipError_t ce = hipStreamEndCapture(net->stream, &g);
  for (void* p : cap.deferred) (void)hipFree(p);
  (void)hipGetLastError();
  hipGraphExec_t exec = nullptr;
  if (rc == TN_OK && (ce != hipSuccess || !g || cap.spilled)) rc = TN_ERR_HIP;
  if (rc == TN_OK &&
      hipGraphInstantiate(&exec, g, nullptr, nullptr, 0) != hipSuccess) {
    (void)hipGetLastError();
    rc = TN_ERR_HIP;
  }
  if (g) (void)hipGraphDestroy(g);
  if (rc != TN_OK) {
    S.graph_state = -1;
    return rc;
  }
  S.graph_exec = exec;
  S.graph_state = 2;
  S.graph_acc = acc;
  return TN_OK;
}

// all listed assignments, then the one wait that closes the call. The rules
// of tn_net_contract: first run normal, second captured, later ones replayed.
static int sliced_loop(tn_net* net, SliceState& S, size_t nwhich, void* acc,
                       hipEvent_t e0, hipEvent_t e1, double* elapsed_ms) {
  HIP_CHECK(hipEventRecord(e0, net->stream));
  for (size_t k = 0; k < nwhich; ++k) {
    HIP_CHECK(hipMemcpyAsync(S.ctl, (const SliceCtl*)S.table + k,
                             sizeof(SliceCtl), hipMemcpyDeviceToDevice,
                             net->stream));
    // the graph writes to the accumulator it was captured with
    if (S.graph_state == 2 && S.graph_acc != acc) S.drop_graph();
    if (S.graph_state == 1 && net->arena.base)
      (void)sliced_capture(net, S, acc);
    if (S.graph_state == 2) {
      if (hipGraphLaunch(S.graph_exec, net->stream) != hipSuccess) {
        (void)hipGetLastError();
        S.drop_graph();
        S.graph_state = -1;
        FAILV(TN_ERR_HIP, "hipGraphLaunch failed");
      }
      continue;
    }
    if (int rc = sliced_unit(net, S, acc, nullptr)) return rc;
    if (S.graph_state == 0 && net->arena.base) S.graph_state = 1;
  }
  HIP_CHECK(hipEventRecord(e1, net->stream));
  HIP_CHECK(hipStreamSynchronize(net->stream));
  float ms = 0.f;
  HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  if (elapsed_ms) *elapsed_ms = (double)ms;
  return TN_OK;
}

extern "C" int tn_net_contract_sliced(tn_net* net, const u64* pairs,
                                      size_t nsteps, const u64* slice_labels,
                                      size_t nlabels, const u64* which,
                                      size_t nwhich, double* elapsed_ms) {
  if (!net) FAILV(TN_ERR_INVALID, "null net");
  if (!which || nwhich == 0)
    FAILV(TN_ERR_INVALID, "no slice assignment listed");
  if ((nsteps && !pairs) || (nlabels && !slice_labels))
    FAILV(TN_ERR_INVALID, "null pairs or slice labels");
  if (net->leaves.size() != nsteps + 1)
    FAILV(TN_ERR_INVALID, "path did not fully contract the network");
  HIP_CHECK(hipSetDevice(net->device));
  SliceState* S = nullptr;
  if (int rc = slice_state(net, pairs, nsteps, slice_labels, nlabels, &S))
    return rc;
  for (size_t k = 0; k < nwhich; ++k)
    if (which[k] >= S->plan.count)
      FAILV(TN_ERR_INVALID,
            "slice assignment %llu out of range (%llu assignments)",
            (unsigned long long)which[k], (unsigned long long)S->plan.count);
  net->drop_graph();  // the unsliced graph's blocks are this walk's to take
  release_final(net);

  // per-call control table: entry k sets up the k-th listed assignment
  if (S->table_cap < nwhich) {
    if (S->table) (void)hipFree(S->table);
    S->table = nullptr;
    S->table_cap = 0;
    HIP_CHECK(hipMalloc(&S->table, nwhich * sizeof(SliceCtl)));
    S->table_cap = nwhich;
  }
  std::vector<SliceCtl> table(nwhich);
  for (size_t k = 0; k < nwhich; ++k) table[k] = {which[k], k == 0 ? 1u : 0u};
  HIP_CHECK(hipMemcpy(S->table, table.data(), nwhich * sizeof(SliceCtl),
                      hipMemcpyHostToDevice));

  // the accumulator: the final tensor of the reduced walk, in its order
  DevTensor f;
  static_cast<LayoutTensor&>(f) =
      nsteps ? S->plan.layout.out[nsteps - 1] : S->plan.reduced[0];
  for (u64 d : f.dims) f.elems *= d;
  WsCtx ws{net->arena.base ? &net->arena : nullptr, net->stream};
  if (ws_alloc(ws, &f.data, f.elems * net->esize) != TN_OK)
    FAILV(TN_ERR_OOM, "device allocation failed for the accumulator");
  hipEvent_t e0 = nullptr, e1 = nullptr;
  int rc = TN_OK;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
    g_last_error = "hipEventCreate failed";
    rc = TN_ERR_HIP;
  }
  if (rc == TN_OK) rc = sliced_loop(net, *S, nwhich, f.data, e0, e1, elapsed_ms);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (rc != TN_OK) {
    (void)hipStreamSynchronize(net->stream);
    ws_free(ws, f.data);
    return rc;
  }
  f.owned = true;
  net->final_in_arena = net->arena.owns(f.data);
  net->final_t = std::move(f);
  net->has_final = true;
  return TN_OK;
}

extern "C" int tn_memcpy_dtod(void* dst, const void* src, u64 bytes) {
  HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice));
  return TN_OK;
}

extern "C" int tn_memcpy_dtoh(void* host_dst, const void* dev_src,
                              u64 bytes) {
  HIP_CHECK(hipMemcpy(host_dst, dev_src, bytes, hipMemcpyDeviceToHost));
  return TN_OK;
}

extern "C" int tn_net_result_meta(tn_net* net, u64* labels, u64* dims,
                                  size_t* ndim) {
  if (!net || !net->has_final) FAILV(TN_ERR_INVALID, "no result available");
  size_t nd = net->final_t.labels.size();
  *ndim = nd;
  for (size_t i = 0; i < nd; ++i) {
    labels[i] = net->final_t.labels[i];
    dims[i] = net->final_t.dims[i];
  }
  return TN_OK;
}

extern "C" int tn_net_result_data(tn_net* net, void* host_out) {
  if (!net || !net->has_final) FAILV(TN_ERR_INVALID, "no result available");
  HIP_CHECK(hipSetDevice(net->device));
  HIP_CHECK(hipMemcpy(host_out, net->final_t.data,
                      net->final_t.elems * net->esize,
                      hipMemcpyDeviceToHost));
  return TN_OK;
}

extern "C" void* tn_net_result_dev(tn_net* net) {
  if (!net || !net->has_final) return nullptr;
  return net->final_t.data;
}

extern "C" int tn_net_pool_bytes(tn_net* net, u64* in_use, u64* cached) {
  if (!net) FAILV(TN_ERR_INVALID, "null net");
  // arena telemetry (the stream-ordered pool is unused — see ws_alloc)
  u64 used = 0;
  for (const auto& b : net->arena.blocks)
    if (!b.free) used += b.sz;
  if (in_use) *in_use = used;
  if (cached) *cached = net->arena.size;
  return TN_OK;
}

extern "C" int tn_net_replay_state(tn_net* net, int32_t* plain,
                                   int32_t* sliced) {
  if (!net) FAILV(TN_ERR_INVALID, "null net");
  if (plain) *plain = net->graph_state;
  if (sliced) *sliced = net->slices ? net->slices->graph_state : 0;
  return TN_OK;
}

extern "C" void tn_net_destroy(tn_net* net) {
  if (!net) return;
  (void)hipSetDevice(net->device);
  (void)hipStreamSynchronize(net->stream);
  net->invalidate_graph();
  for (auto& t : net->leaves)
    if (t.data && !t.owned && !t.external) (void)hipFree(t.data);
  if (net->has_final && net->final_t.owned && !net->final_in_arena)
    (void)hipFree(net->final_t.data);
  net->arena.destroy();
  (void)hipStreamDestroy(net->stream);
  if (net->stream2) (void)hipStreamDestroy(net->stream2);
  delete net;
}

// ---------------------------------------------------------------------------
// sampling: flat indices of a contiguous complex tensor drawn with
// probability |T[i]|^2 (semantics: include/tnc_hip.h, step_plan.hpp). Three
// launches: chunk sums (the one pass over the tensor, HBM-bound), their
// sequential prefix in one block, one block per shot that bisects the prefix
// and scans one chunk out of LDS.
// ---------------------------------------------------------------------------

// p = re^2 + im^2 in f64: two products and one add, never a fused
// multiply-add, so pass 1, the draw and a host reference round alike
template <typename RT>
__device__ __forceinline__ double sample_prob(RT re, RT im) {
#pragma clang fp contract(off)
  const double a = (double)re * (double)re;
  const double b = (double)im * (double)im;
  return a + b;
}

// p of element e of a full chunk lands in v[]: 16-byte loads, lane-contiguous.
// c128: load it holds element it*256+tid. c64: load it holds elements
// 2*(it*256+tid) and the one after it.
template <typename CT>
struct SampleLoad;

template <>
struct SampleLoad<double2> {
  static constexpr int LOADS = TN_SAMPLE_CHUNK / TN_SAMPLE_THREADS;
  static constexpr int PER = 1;
  typedef double2 Vec;
  static __device__ __forceinline__ void probs(const Vec& v, double* p) {
    p[0] = sample_prob(v.x, v.y);
  }
};

template <>
struct SampleLoad<float2> {
  static constexpr int LOADS = TN_SAMPLE_CHUNK / TN_SAMPLE_THREADS / 2;
  static constexpr int PER = 2;
  typedef float4 Vec;
  static __device__ __forceinline__ void probs(const Vec& v, double* p) {
    p[0] = sample_prob(v.x, v.y);
    p[1] = sample_prob(v.z, v.w);
  }
};

// S[j] = sum of p over chunk j = blockIdx.x. Fixed order: each lane adds its
// loads in load order, lanes are added by xor-shuffles, waves one after
// another. A short last chunk goes element by element.
template <typename CT>
__global__ __launch_bounds__(TN_SAMPLE_THREADS) void k_prob_chunk_sums(
    const CT* __restrict__ T, double* __restrict__ S, u64 n) {
  typedef SampleLoad<CT> LD;
  __shared__ double sred[TN_SAMPLE_THREADS / 64];
  const int tid = threadIdx.x;
  const u64 base = (u64)blockIdx.x * TN_SAMPLE_CHUNK;
  const u64 len = n - base < TN_SAMPLE_CHUNK ? n - base : TN_SAMPLE_CHUNK;
  const CT* src = T + base;
  double acc = 0.0;
  if (len == TN_SAMPLE_CHUNK) {
    const typename LD::Vec* srcv =
        reinterpret_cast<const typename LD::Vec*>(src);
    typename LD::Vec v[LD::LOADS];
#pragma unroll
    for (int it = 0; it < LD::LOADS; ++it)
      v[it] = srcv[it * TN_SAMPLE_THREADS + tid];
#pragma unroll
    for (int it = 0; it < LD::LOADS; ++it) {
      double p[LD::PER];
      LD::probs(v[it], p);
#pragma unroll
      for (int x = 0; x < LD::PER; ++x) acc += p[x];
    }
  } else {
    for (u64 e = tid; e < len; e += TN_SAMPLE_THREADS) {
      const CT v = src[e];
      acc += sample_prob(v.x, v.y);
    }
  }
  for (int s = 32; s > 0; s >>= 1) acc += __shfl_xor(acc, s, 64);
  if ((tid & 63) == 0) sred[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double tot = sred[0];
    for (int w = 1; w < TN_SAMPLE_THREADS / 64; ++w) tot += sred[w];
    S[blockIdx.x] = tot;
  }
}

// C[j] = C[j-1] + S[j] in place, one add after another in ascending j: the
// association is part of the semantics, so one thread adds. The block only
// moves the entries through LDS, TILE per pass. (A template, so that it is
// placed in the code object where it is first used, behind the kernels that
// were there before it.)
template <int TILE>
__global__ __launch_bounds__(TN_SAMPLE_THREADS) void k_prob_scan(
    double* __restrict__ SC, u64 nchunks, double* __restrict__ total) {
  constexpr int B = 16;  // entries thread 0 holds in registers at a time
  constexpr int PER = TILE / TN_SAMPLE_THREADS;  // entries a thread moves
  static_assert(TILE % B == 0 && TILE % TN_SAMPLE_THREADS == 0, "whole");
  __shared__ double tile[TILE];
  const int tid = threadIdx.x;
  // One block hides no latency behind other blocks: a thread's entries of
  // the next tile are loaded into v[] while thread 0 adds up this one.
  // Entries past the end are zeros: adding them leaves run as it is.
  double v[PER];
  auto load = [&](u64 base) {
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const u64 e = base + (u64)(k * TN_SAMPLE_THREADS + tid);
      v[k] = e < nchunks ? SC[e] : 0.0;
    }
  };
  load(0);
  double run = 0.0;  // thread 0's
  for (u64 base = 0; base < nchunks; base += TILE) {
    const int len = nchunks - base < TILE ? (int)(nchunks - base) : TILE;
    const int padded = (len + B - 1) / B * B;
#pragma unroll
    for (int k = 0; k < PER; ++k) tile[k * TN_SAMPLE_THREADS + tid] = v[k];
    __syncthreads();
    if (base + TILE < nchunks) load(base + TILE);
    if (tid == 0) {
      // the adds are one dependent chain; the LDS reads of the next batch
      // are issued ahead of it so that only the adds are waited for
      double cur[B], nxt[B];
#pragma unroll
      for (int i = 0; i < B; ++i) cur[i] = tile[i];
      for (int b = 0; b < padded; b += B) {
        if (b + B < padded) {
#pragma unroll
          for (int i = 0; i < B; ++i) nxt[i] = tile[b + B + i];
        }
#pragma unroll
        for (int i = 0; i < B; ++i) {
          run += cur[i];
          tile[b + i] = run;
        }
#pragma unroll
        for (int i = 0; i < B; ++i) cur[i] = nxt[i];
      }
    }
    __syncthreads();
    // each thread stores the entries it wrote and will overwrite next pass
    for (int e = tid; e < len; e += TN_SAMPLE_THREADS) SC[base + e] = tile[e];
  }
  if (tid == 0) *total = run;
}

// One shot per block: restates sample_pick_chunk and sample_pick_in_chunk
// (step_plan.hpp). The chunk's p values go to LDS with one pad double per
// slab, so that the per-thread slab reads spread over the banks.
template <typename CT>
__global__ __launch_bounds__(TN_SAMPLE_THREADS) void k_sample_draw(
    const CT* __restrict__ T, u64 n, const double* __restrict__ C,
    u64 nchunks, const double* __restrict__ total,
    const double* __restrict__ u, u64* __restrict__ idx) {
  typedef SampleLoad<CT> LD;
  constexpr int STRIDE = TN_SAMPLE_SLAB + 1;
  __shared__ double sp[TN_SAMPLE_THREADS * STRIDE];
  __shared__ double sslab[TN_SAMPLE_THREADS];
  __shared__ int sfirst[TN_SAMPLE_THREADS / 64], slast[TN_SAMPLE_THREADS / 64];
  const int tid = threadIdx.x;
  const double t = u[blockIdx.x] * *total;

  // sample_pick_chunk, the same in every thread
  u64 lo = 0, hi = nchunks;
  while (lo < hi) {
    const u64 mid = lo + (hi - lo) / 2;
    if (C[mid] > t)
      hi = mid;
    else
      lo = mid + 1;
  }
  if (lo == nchunks) {
    const double top = C[nchunks - 1];
    lo = 0, hi = nchunks - 1;
    while (lo < hi) {
      const u64 mid = lo + (hi - lo) / 2;
      if (C[mid] < top)
        lo = mid + 1;
      else
        hi = mid;
    }
  }
  const u64 j = lo;
  const double tp = t - (j ? C[j - 1] : 0.0);

  // the chunk's p, zero past the end of a short last chunk
  const u64 base = j * TN_SAMPLE_CHUNK;
  const u64 len = n - base < TN_SAMPLE_CHUNK ? n - base : TN_SAMPLE_CHUNK;
  const CT* src = T + base;
  if (len == TN_SAMPLE_CHUNK) {
    const typename LD::Vec* srcv =
        reinterpret_cast<const typename LD::Vec*>(src);
    typename LD::Vec v[LD::LOADS];
#pragma unroll
    for (int it = 0; it < LD::LOADS; ++it)
      v[it] = srcv[it * TN_SAMPLE_THREADS + tid];
#pragma unroll
    for (int it = 0; it < LD::LOADS; ++it) {
      double p[LD::PER];
      LD::probs(v[it], p);
#pragma unroll
      for (int x = 0; x < LD::PER; ++x) {
        const int e = (it * TN_SAMPLE_THREADS + tid) * LD::PER + x;
        sp[e + e / TN_SAMPLE_SLAB] = p[x];
      }
    }
  } else {
    for (int e = tid; e < TN_SAMPLE_CHUNK; e += TN_SAMPLE_THREADS) {
      double p = 0.0;
      if ((u64)e < len) {
        const CT v = src[e];
        p = sample_prob(v.x, v.y);
      }
      sp[e + e / TN_SAMPLE_SLAB] = p;
    }
  }
  __syncthreads();

  // sample_pick_in_chunk: own slab from zero, the slab sums in front added
  // one after another, then the slab's elements added to that in order
  double v[TN_SAMPLE_SLAB];
  double slab = 0.0;
#pragma unroll
  for (int i = 0; i < TN_SAMPLE_SLAB; ++i) {
    v[i] = sp[tid * STRIDE + i];
    slab += v[i];
  }
  sslab[tid] = slab;
  __syncthreads();
  double r = 0.0;
  for (int k = 0; k < tid; ++k) r += sslab[k];
  int first = TN_SAMPLE_CHUNK, last = -1;
#pragma unroll
  for (int i = 0; i < TN_SAMPLE_SLAB; ++i) {
    r += v[i];
    if (v[i] > 0.0) {
      last = tid * TN_SAMPLE_SLAB + i;
      if (first == TN_SAMPLE_CHUNK && r > tp) first = last;
    }
  }
  for (int s = 32; s > 0; s >>= 1) {
    first = min(first, __shfl_xor(first, s, 64));
    last = max(last, __shfl_xor(last, s, 64));
  }
  if ((tid & 63) == 0) {
    sfirst[tid >> 6] = first;
    slast[tid >> 6] = last;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < TN_SAMPLE_THREADS / 64; ++w) {
      first = min(first, sfirst[w]);
      last = max(last, slast[w]);
    }
    const int i = first < TN_SAMPLE_CHUNK ? first : (last >= 0 ? last : 0);
    idx[blockIdx.x] = base + (u64)i;
  }
}

extern "C" int tn_plan_sample(u64 n, u64 nshots, int dtype,
                              tn_sample_plan* out) {
  if (dtype != 0 && dtype != 1)
    FAILV(TN_ERR_INVALID, "dtype must be 0 (c128) or 1 (c64)");
  if (!out) FAILV(TN_ERR_INVALID, "null plan");
  SamplePlan sp;
  plan_sample(n, nshots, dtype == 0 ? 16 : 8, &sp);
  if (!sp.valid) FAILV(TN_ERR_INVALID, "%s", sp.err.c_str());
  out->chunk = sp.chunk;
  out->nchunks = sp.nchunks;
  out->grid_sums = sp.grid_sums;
  out->grid_scan = sp.grid_scan;
  out->grid_draw = sp.grid_draw;
  out->ws_bytes = sp.ws_bytes;
  return TN_OK;
}

// passes 1 and 2: C[nchunks] and *total
template <typename CT>
static int sample_launch_sums(const SamplePlan& sp, const void* data, u64 n,
                              double* C, double* total, hipStream_t stream) {
  k_prob_chunk_sums<CT><<<dim3((unsigned)sp.grid_sums), TN_SAMPLE_THREADS, 0,
                          stream>>>((const CT*)data, C, n);
  k_prob_scan<TN_SAMPLE_SCAN_TILE><<<dim3((unsigned)sp.grid_scan),
                                     TN_SAMPLE_THREADS, 0, stream>>>(
      C, sp.nchunks, total);
  HIP_CHECK(hipGetLastError());
  return TN_OK;
}

template <typename CT>
static int sample_launch_draw(const SamplePlan& sp, const void* data, u64 n,
                              const double* C, const double* total,
                              const double* u, u64* idx, hipStream_t stream) {
  if (!sp.grid_draw) return TN_OK;
  k_sample_draw<CT><<<dim3((unsigned)sp.grid_draw), TN_SAMPLE_THREADS, 0,
                      stream>>>((const CT*)data, n, C, sp.nchunks, total, u,
                                idx);
  HIP_CHECK(hipGetLastError());
  return TN_OK;
}

template <typename CT>
static int sample_dev_impl(const void* data, u64 n, const double* u_dev,
                           u64 nshots, u64* idx_dev, double* norm2_dev,
                           void* ws_dev, u64 ws_bytes, void* stream) {
  SamplePlan sp;
  plan_sample(n, nshots, sizeof(CT), &sp);
  if (!sp.valid) FAILV(TN_ERR_INVALID, "%s", sp.err.c_str());
  if (!data || !norm2_dev || !ws_dev || (nshots && (!u_dev || !idx_dev)))
    FAILV(TN_ERR_INVALID, "null pointer");
  if ((uintptr_t)data % 16 || (uintptr_t)ws_dev % 8)
    FAILV(TN_ERR_INVALID,
          "data must be 16-byte aligned and the workspace 8-byte aligned");
  if (ws_bytes < sp.off_u)
    FAILV(TN_ERR_INVALID, "workspace of %llu bytes, %llu needed",
          (unsigned long long)ws_bytes, (unsigned long long)sp.off_u);
  hipStream_t s = (hipStream_t)stream;
  if (int rc = sample_launch_sums<CT>(sp, data, n, (double*)ws_dev, norm2_dev,
                                      s))
    return rc;
  return sample_launch_draw<CT>(sp, data, n, (const double*)ws_dev, norm2_dev,
                                u_dev, idx_dev, s);
}

extern "C" int tn_sample_c128_dev(const void* data, u64 n,
                                  const double* u_dev, u64 nshots,
                                  u64* idx_dev, double* norm2_dev,
                                  void* ws_dev, u64 ws_bytes, void* stream) {
  return sample_dev_impl<double2>(data, n, u_dev, nshots, idx_dev, norm2_dev,
                                  ws_dev, ws_bytes, stream);
}

extern "C" int tn_sample_c64_dev(const void* data, u64 n, const double* u_dev,
                                 u64 nshots, u64* idx_dev, double* norm2_dev,
                                 void* ws_dev, u64 ws_bytes, void* stream) {
  return sample_dev_impl<float2>(data, n, u_dev, nshots, idx_dev, norm2_dev,
                                 ws_dev, ws_bytes, stream);
}

extern "C" int tn_net_sample(tn_net* net, const double* u_host, u64 nshots,
                             u64* idx_host, double* norm2) {
  if (!net || !net->has_final || !net->final_t.data)
    FAILV(TN_ERR_INVALID, "no final tensor to sample: contract first");
  const u64 n = net->final_t.elems;
  if (n == 0) FAILV(TN_ERR_INVALID, "final tensor has no elements");
  if (nshots && (!u_host || !idx_host))
    FAILV(TN_ERR_INVALID, "null pointer");
  for (u64 s = 0; s < nshots; ++s)
    if (!(u_host[s] >= 0.0 && u_host[s] < 1.0))
      FAILV(TN_ERR_INVALID, "u[%llu] = %.17g is outside [0, 1)",
            (unsigned long long)s, u_host[s]);
  SamplePlan sp;
  plan_sample(n, nshots, net->esize, &sp);
  if (!sp.valid) FAILV(TN_ERR_INVALID, "%s", sp.err.c_str());
  HIP_CHECK(hipSetDevice(net->device));
  // one block, from the arena when there is one, never from the
  // stream-ordered pool (ws_alloc); released on every way out of here
  WsCtx ws{net->arena.base ? &net->arena : nullptr, net->stream};
  WsBlock<char> blk(ws);
  if (int rc = blk.alloc(sp.ws_bytes)) return rc;
  double* C = (double*)blk.p;
  double* u_dev = (double*)(blk.p + sp.off_u);
  u64* idx_dev = (u64*)(blk.p + sp.off_idx);
  double* total_dev = (double*)(blk.p + sp.off_total);
  const void* data = net->final_t.data;
  const bool c128 = net->dtype == 0;
  int rc = c128 ? sample_launch_sums<double2>(sp, data, n, C, total_dev,
                                              net->stream)
                : sample_launch_sums<float2>(sp, data, n, C, total_dev,
                                             net->stream);
  if (rc) {
    (void)hipStreamSynchronize(net->stream);
    return rc;
  }
  // the block goes back to the arena only once nothing in flight uses it
  hipError_t err = hipStreamSynchronize(net->stream);
  double total = 0.0;
  if (err == hipSuccess)
    err = hipMemcpy(&total, total_dev, sizeof total, hipMemcpyDeviceToHost);
  HIP_CHECK(err);
  if (norm2) *norm2 = total;
  if (total == 0.0) FAILV(TN_ERR_INVALID, "final tensor has zero norm");
  if (!(total - total == 0.0))
    FAILV(TN_ERR_INVALID, "final tensor norm is not finite");
  if (!nshots) return TN_OK;
  HIP_CHECK(hipMemcpy(u_dev, u_host, nshots * 8, hipMemcpyHostToDevice));
  rc = c128 ? sample_launch_draw<double2>(sp, data, n, C, total_dev, u_dev,
                                          idx_dev, net->stream)
            : sample_launch_draw<float2>(sp, data, n, C, total_dev, u_dev,
                                         idx_dev, net->stream);
  err = hipStreamSynchronize(net->stream);
  if (rc) return rc;
  HIP_CHECK(err);
  HIP_CHECK(hipMemcpy(idx_host, idx_dev, nshots * 8, hipMemcpyDeviceToHost));
  return TN_OK;
}
