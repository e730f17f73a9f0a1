// Stand-alone host replay of the addressing of the two tiled bit-permutation
// kernels, k_permute_tile and k_dot_tile, from the plans the executor hands
// them (plan_permute_tile / plan_dot_tile). Needs only a host compiler, e.g.
//   g++ -std=c++17 -O1 -g -Wall -fsanitize=address,undefined
//       -fno-sanitize-recover=undefined tests/native/tile_perm_check.cpp
// Exit 0 and "tile_perm_check OK" on success.
//
// k_permute_tile: every address is formed as the kernel forms it (rest bits
// from the block index, the sboffS / sboffD / saoffD tables, the swizzled LDS
// slot, a, b). Every source read stays inside the source span, every
// destination is in bounds and hit exactly once, and dst[p] reads
// src[gather(p)] for the row-major p of the axis list.
// k_dot_tile: every (block, b, lane) pair of A and B offsets names the same
// K multi-index, and every K index is visited exactly once on both sides.
// After each passing replay one plan entry is swapped (two aD entries, two
// restB entries) and the replay must then report a mismatch: the check can
// fail.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../tnc_amd/csrc/step_plan.hpp"

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, \
              #cond);                                                \
      exit(1);                                                       \
    }                                                                \
  } while (0)

typedef std::vector<u64> Legs;

static Legs legs(u64 base, int count) {
  Legs v;
  for (int x = 0; x < count; ++x) v.push_back(base + x);
  return v;
}

static Legs cat(std::initializer_list<Legs> parts) {
  Legs v;
  for (const Legs& p : parts) v.insert(v.end(), p.begin(), p.end());
  return v;
}

static Legs reversed(Legs v) {
  std::reverse(v.begin(), v.end());
  return v;
}

// fixed shuffle (Fisher-Yates over a 64-bit LCG): the same on every machine
static Legs shuffled(Legs v, u64 seed) {
  for (size_t i = v.size(); i > 1; --i) {
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    std::swap(v[i - 1], v[(seed >> 33) % i]);
  }
  return v;
}

static LayoutTensor tensor(const Legs& l, const Legs& d = Legs()) {
  LayoutTensor t;
  t.labels = l;
  t.dims = d.empty() ? Legs(l.size(), 2) : d;
  CHECK(t.labels.size() == t.dims.size());
  return t;
}

// axis list of the permute src (contiguous row-major, may hold labels that
// dst lacks: those stay fixed, a sub-box) -> dst order
static std::vector<AxisInfo> axes_of(const LayoutTensor& src,
                                     const Legs& dst) {
  Meta m;
  layout_meta(src, &m);
  std::vector<AxisInfo> ax;
  for (u64 lab : dst) {
    int at = -1;
    for (int i = 0; i < m.nd; ++i)
      if (m.labels[i] == lab) at = i;
    CHECK(at >= 0);
    ax.push_back({m.dims[at], m.strides[at], 0});
  }
  return ax;
}

static u64 elems_of(const std::vector<AxisInfo>& ax) {
  u64 n = 1;
  for (const AxisInfo& a : ax) n *= a.dim;
  return n;
}

// ---- k_permute_tile -------------------------------------------------------

// Replays every block of k_permute_tile<<<1 << pp.rbits, 512>>>. Returns
// false on the first address that is out of bounds, hit twice or not the
// gather of its row-major destination index.
static bool replay_permute(const std::vector<AxisInfo>& ax,
                           const PermPerm& pp, bool verbose) {
  constexpr int AN = 1 << TN_PERM_AB, BN = 1 << TN_PERM_BB;
  const u64 elems = elems_of(ax);
  u64 span = 1;  // source elements the gather may touch
  for (const AxisInfo& a : ax) span += (a.dim - 1) * (u64)a.sa;
  auto fail = [&](const char* what, u64 v) {
    if (verbose) fprintf(stderr, "permute replay: %s (%llu)\n", what,
                         (unsigned long long)v);
    return false;
  };
  if (pp.rbits < 0 || pp.rbits > TN_PERM_MAXBITS) return fail("rbits", 0);
  if ((1ull << (pp.rbits + TN_PERM_AB + TN_PERM_BB)) != elems)
    return fail("grid does not cover the elements", elems);
  // reference: source offset of every row-major destination index
  std::vector<u64> gather(elems);
  for (u64 p = 0; p < elems; ++p) {
    u64 idx = p, off = 0;
    for (int i = (int)ax.size() - 1; i >= 0; --i) {
      off += (idx % ax[i].dim) * (u64)ax[i].sa;
      idx /= ax[i].dim;
    }
    gather[p] = off;
  }
  std::vector<unsigned char> hit(elems, 0);
  u64 sboffS[BN], sboffD[BN], saoffD[AN];
  for (int tid = 0; tid < BN; ++tid) {
    u64 os = 0, od = 0;
    for (int i = 0; i < TN_PERM_BB; ++i)
      if (tid >> i & 1) {
        os += pp.bS[i];
        od += pp.bD[i];
      }
    sboffS[tid] = os;
    sboffD[tid] = od;
  }
  for (int a = 0; a < AN; ++a) {
    u64 od = 0;
    for (int i = 0; i < TN_PERM_AB; ++i)
      if (a >> i & 1) od += pp.aD[i];
    saoffD[a] = od;
  }
  const u64 none = ~0ull;
  std::vector<u64> tile(AN * BN);  // source offset held by each LDS slot
  for (u64 block = 0; block < (1ull << pp.rbits); ++block) {
    u64 baseS = 0, baseD = 0;
    {
      unsigned r = (unsigned)block;
      for (int i = 0; i < pp.rbits; ++i) {
        if (r & 1) {
          baseS += pp.restS[i];
          baseD += pp.restD[i];
        }
        r >>= 1;
      }
    }
    std::fill(tile.begin(), tile.end(), none);
    for (int e = 0; e < AN * BN; ++e) {
      const int a = e & (AN - 1), b = e >> TN_PERM_AB;
      const u64 s = baseS + sboffS[b] + (u64)a;
      if (s >= span) return fail("source read out of bounds", s);
      const int slot = b * AN + ((a ^ b) & (AN - 1));
      if (tile[slot] != none) return fail("LDS slot written twice", slot);
      tile[slot] = s;
    }
    for (int e = 0; e < AN * BN; ++e) {
      const int b = e & (BN - 1), a = e >> TN_PERM_BB;
      const u64 d = baseD + saoffD[a] + sboffD[b];
      if (d >= elems) return fail("destination out of bounds", d);
      if (hit[d]) return fail("destination hit twice", d);
      hit[d] = 1;
      const u64 s = tile[b * AN + ((a ^ b) & (AN - 1))];
      if (s == none) return fail("LDS slot read before written", d);
      if (s != gather[d]) return fail("dst[p] != src[gather(p)] at p", d);
    }
  }
  // 2^rbits blocks of AN*BN distinct in-bounds destinations = all of them
  return true;
}

static void permute_case(const char* name, const std::vector<AxisInfo>& ax,
                         int want_rbits) {
  const u64 elems = elems_of(ax);
  PermPerm pp;
  const int nr = plan_permute_tile(ax, elems, &pp);
  if (nr != want_rbits) {
    fprintf(stderr, "%s: %d rest bits, expected %d\n", name, nr, want_rbits);
    exit(1);
  }
  CHECK(permute_kind(ax, elems) == 2);
  if (!replay_permute(ax, pp, true)) {
    fprintf(stderr, "%s: replay failed\n", name);
    exit(1);
  }
  // self-test: the replay notices two swapped a-bit destination strides
  PermPerm bad = pp;
  std::swap(bad.aD[1], bad.aD[4]);
  CHECK(bad.aD[1] != pp.aD[1]);
  if (replay_permute(ax, bad, false)) {
    fprintf(stderr, "%s: replay passed a perturbed plan\n", name);
    exit(1);
  }
}

static void permute_refused(const char* name, const std::vector<AxisInfo>& ax,
                            u64 elems) {
  PermPerm pp;
  if (plan_permute_tile(ax, elems, &pp) != -1 ||
      permute_kind(ax, elems) != 1) {
    fprintf(stderr, "%s: not refused\n", name);
    exit(1);
  }
}

static void permute_checks() {
  const Legs M = legs(1, 12), K = legs(101, 8);
  // M/K legs interleaved in the source: m1 k1 m2 k2 ... m8 k8 m9..m12
  Legs inter;
  for (int i = 0; i < 12; ++i) {
    inter.push_back(M[i]);
    if (i < 8) inter.push_back(K[i]);
  }
  const Legs mk = cat({M, K});
  permute_case("interleave", axes_of(tensor(inter), mk), 9);
  permute_case("reverse", axes_of(tensor(legs(1, 20)), reversed(legs(1, 20))),
               9);
  // the six lowest source bits stay the six lowest destination bits: the
  // b-bits are then destination bits 6..10
  {
    const Legs lo = legs(301, 6), hi = legs(201, 14);
    permute_case("low6_fixed", axes_of(tensor(cat({hi, lo})),
                                       cat({reversed(hi), lo})), 9);
  }
  // mixed dims 16/64/4: A = [k1:16, m1:64, k2:4, m2:16, k3:4, m3:4] packed to
  // [m3, m1, m2, k1, k2, k3]
  {
    const LayoutTensor a =
        tensor({101, 1, 102, 2, 103, 3}, {16, 64, 4, 16, 4, 4});
    permute_case("mixed", axes_of(a, {3, 1, 2, 101, 102, 103}), 9);
  }
  // a dim-1 axis contributes no bits, whatever its stride
  {
    std::vector<AxisInfo> ax = axes_of(tensor(inter), mk);
    ax.insert(ax.begin() + 5, AxisInfo{1, 0, 0});
    ax.push_back(AxisInfo{1, -3, 0});
    permute_case("dim1", ax, 9);
  }
  // sub-box: one K-window of A = [m2:64, k1:2, m1:64, k2:256] packed to
  // [m2, m1, k2] (and to [m1, m2, k2]); k1 selects the window and leaves a
  // gap in the source span. The window list of case P_subbox in
  // tests/kernel_reach_cases.py.
  {
    const LayoutTensor a = tensor({2, 100, 1, 101}, {64, 2, 64, 256});
    const std::vector<AxisInfo> ax = axes_of(a, {2, 1, 101});
    CHECK(elems_of(ax) == (1ull << 20));
    permute_case("subbox", ax, 9);
    permute_case("subbox_swapped", axes_of(a, {1, 2, 101}), 9);
  }
  // 2^21 elements: ten rest bits
  permute_case("perm21", axes_of(tensor(legs(1, 21)),
                                 shuffled(legs(1, 21), 21)), 10);

  // refusals
  permute_refused("under_2^20", axes_of(tensor(legs(1, 19)),
                                        reversed(legs(1, 19))), 1ull << 19);
  {
    const LayoutTensor a = tensor({1, 2, 3}, {1024, 3, 512});
    permute_refused("non_pow2", axes_of(a, {3, 2, 1}), 3ull << 19);
  }
  {
    std::vector<AxisInfo> ax = axes_of(tensor(legs(1, 20)),
                                       reversed(legs(1, 20)));
    ax[3].sa = -ax[3].sa;
    permute_refused("negative_stride", ax, 1ull << 20);
    ax[3].sa = 0;
    permute_refused("zero_stride", ax, 1ull << 20);
  }
  {
    // eleven bits claiming 2^20 elements (the list and the count disagree),
    // and a list of exactly eleven bits
    const std::vector<AxisInfo> ax =
        axes_of(tensor(legs(1, 11)), reversed(legs(1, 11)));
    permute_refused("eleven_bits", ax, 1ull << 20);
    permute_refused("eleven_bits_exact", ax, 1ull << 11);
  }
  {
    // lowest source strides 2..64 (the stride-1 leg 21 stays fixed): a
    // strided view, no coalesced 64-run
    std::vector<AxisInfo> ax = axes_of(tensor(legs(1, 21)),
                                       reversed(legs(1, 20)));
    permute_refused("low_strides", ax, 1ull << 20);
  }
}

// ---- k_dot_tile -----------------------------------------------------------

struct DotCase {
  Meta A, B;
  AxisList k_a, k_b;
  u64 K;
};

static DotCase dot_case(const LayoutTensor& a, const Legs& b_order) {
  DotCase c;
  LayoutTensor b;
  for (u64 lab : b_order)
    for (size_t i = 0; i < a.labels.size(); ++i)
      if (a.labels[i] == lab) {
        b.labels.push_back(lab);
        b.dims.push_back(a.dims[i]);
      }
  CHECK(b.labels.size() == a.labels.size());
  layout_meta(a, &c.A);
  layout_meta(b, &c.B);
  c.K = 1;
  for (int i = 0; i < c.A.nd; ++i) {
    c.K *= c.A.dims[i];
    for (int j = 0; j < c.B.nd; ++j)
      if (c.B.labels[j] == c.A.labels[i]) {
        c.k_a.push_back(i);
        c.k_b.push_back(j);
      }
  }
  return c;
}

// Replays k_dot_tile<CT, TN_DOT_TILE_BBITS><<<1 << dp.rbits, 512>>>.
static bool replay_dot(const DotCase& c, const DotPerm& dp, bool verbose) {
  constexpr int BB = TN_DOT_TILE_BBITS, NB = 1 << BB;
  const u64 K = c.K;
  auto fail = [&](const char* what, u64 v) {
    if (verbose) fprintf(stderr, "dot replay: %s (%llu)\n", what,
                         (unsigned long long)v);
    return false;
  };
  if (dp.rbits < 0 || dp.rbits > TN_DOT_MAXBITS) return fail("rbits", 0);
  if ((1ull << (dp.rbits + TN_DOT_TILE_BITS)) != K)
    return fail("grid does not cover K", K);
  u64 sboffA[NB], sboffB[NB], saoffB[64];
  for (int tid = 0; tid < NB; ++tid) {
    u64 oa = 0, ob = 0;
    for (int i = 0; i < BB; ++i)
      if (tid >> i & 1) {
        oa += dp.bA[i];
        ob += dp.bB[i];
      }
    sboffA[tid] = oa;
    sboffB[tid] = ob;
  }
  for (int a = 0; a < 64; ++a) {
    u64 ob = 0;
    for (int i = 0; i < TN_DOT_TILE_ABITS; ++i)
      if (a >> i & 1) ob += dp.aB[i];
    saoffB[a] = ob;
  }
  std::vector<unsigned char> hitA(K, 0), hitB(K, 0);
  const u64 none = ~0ull;
  std::vector<u64> tile(NB * 64);  // B offset held by each LDS slot
  for (u64 block = 0; block < (1ull << dp.rbits); ++block) {
    u64 baseA = 0, baseB = 0;
    {
      unsigned r = (unsigned)block;
      for (int i = 0; i < dp.rbits; ++i) {
        if (r & 1) {
          baseA += dp.restA[i];
          baseB += dp.restB[i];
        }
        r >>= 1;
      }
    }
    std::fill(tile.begin(), tile.end(), none);
    for (int e = 0; e < NB * 64; ++e) {
      const int b = e & (NB - 1), a = e >> BB;
      const u64 ob = baseB + saoffB[a] + sboffB[b];
      if (ob >= K) return fail("B read out of bounds", ob);
      const int slot = b * 64 + (a ^ (b & 63));
      if (tile[slot] != none) return fail("LDS slot written twice", slot);
      tile[slot] = ob;
    }
    for (int b = 0; b < NB; ++b)
      for (int lane = 0; lane < 64; ++lane) {
        const u64 oa = baseA + sboffA[b] + (u64)lane;
        if (oa >= K) return fail("A read out of bounds", oa);
        const u64 ob = tile[b * 64 + (lane ^ (b & 63))];
        if (ob == none) return fail("LDS slot read before written", oa);
        if (hitA[oa]) return fail("A element visited twice", oa);
        if (hitB[ob]) return fail("B element visited twice", ob);
        hitA[oa] = hitB[ob] = 1;
        // the same K multi-index on both sides
        for (int t = 0; t < c.k_a.n; ++t) {
          const u64 dim = c.A.dims[c.k_a[t]];
          const u64 ia = oa / (u64)c.A.strides[c.k_a[t]] % dim;
          const u64 ib = ob / (u64)c.B.strides[c.k_b[t]] % dim;
          if (ia != ib) return fail("A and B name different K indices", oa);
        }
      }
  }
  // 2^rbits blocks of 4096 distinct in-bounds offsets per side = all of K
  return true;
}

static void dot_ok(const char* name, const DotCase& c) {
  DotPerm dp;
  const int nr = plan_dot_tile(c.A, c.B, c.k_a, c.k_b, &dp);
  int kbits = 0;
  while ((1ull << kbits) < c.K) ++kbits;
  if (nr != kbits - TN_DOT_TILE_BITS) {
    fprintf(stderr, "%s: %d rest bits, expected %d\n", name, nr,
            kbits - TN_DOT_TILE_BITS);
    exit(1);
  }
  if (!replay_dot(c, dp, true)) {
    fprintf(stderr, "%s: replay failed\n", name);
    exit(1);
  }
  // self-test: the replay notices two swapped rest-bit strides of B
  DotPerm bad = dp;
  std::swap(bad.restB[0], bad.restB[nr - 1]);
  CHECK(bad.restB[0] != dp.restB[0]);
  if (replay_dot(c, bad, false)) {
    fprintf(stderr, "%s: replay passed a perturbed plan\n", name);
    exit(1);
  }
}

static void dot_refused(const char* name, const DotCase& c) {
  DotPerm dp;
  if (plan_dot_tile(c.A, c.B, c.k_a, c.k_b, &dp) != -1) {
    fprintf(stderr, "%s: not refused\n", name);
    exit(1);
  }
}

static void dot_checks() {
  const Legs L = legs(1, 20);
  dot_ok("dot_reverse", dot_case(tensor(L), reversed(L)));
  dot_ok("dot_shuffle", dot_case(tensor(L), shuffled(L, 7)));
  dot_ok("dot_mixed", dot_case(tensor({0, 1, 2, 3, 4, 5, 6},
                                      {4, 8, 2, 16, 4, 64, 4}),
                               {6, 3, 0, 2, 5, 4, 1}));
  dot_ok("dot_2^21", dot_case(tensor(legs(1, 21)), shuffled(legs(1, 21), 3)));
  // a dim-1 leg contributes no bits
  dot_ok("dot_dim1", dot_case(tensor(cat({L, {99}}),
                                     cat({Legs(20, 2), {1}})),
                              cat({{99}, reversed(L)})));

  // refusals
  dot_refused("dot_non_pow2", dot_case(tensor({1, 2, 3}, {1024, 3, 512}),
                                       {3, 2, 1}));
  dot_refused("dot_twelve_bits", dot_case(tensor(legs(1, 12)),
                                          reversed(legs(1, 12))));
  {
    DotCase c = dot_case(tensor(L), reversed(L));
    c.B.strides[c.k_b[4]] = -c.B.strides[c.k_b[4]];
    dot_refused("dot_negative_stride", c);
    c.B.strides[c.k_b[4]] = 0;
    dot_refused("dot_zero_stride", c);
  }
  {
    // A is a strided view: its span has a gap, no contiguous 2^20 run
    DotCase c = dot_case(tensor(L), reversed(L));
    c.A.strides[0] *= 2;
    dot_refused("dot_gap", c);
  }
}

int main() {
  permute_checks();
  dot_checks();
  printf("tile_perm_check OK\n");
  return 0;
}
