// Stand-alone host check of the gather route's index maps and kernel choice
// (GatherMap, build_map, plan_gather_kernel: step_plan.hpp). Needs only a
// host compiler, e.g.
//   g++ -std=c++17 -O1 -g -Wall -fsanitize=address,undefined
//       -fno-sanitize-recover=undefined tests/native/gather_map_check.cpp
// Exit 0 and "gather_map_check OK" on success.
//
// Maps: the decode of k_einsum_smallk / k_einsum_anyk / k_permute_ct (gather2
// in the HIP file) is re-stated here for both encodings, div/mod and
// shift/mask. For the out and K axis lists of the reach table's gather cases
// (built by plan_step and the executor's own axis-list builders) and for
// seeded random lists, every packed index must decode to the (A offset, B
// offset) of a plain mixed-radix loop. build_map refuses rank > TN_MAXR.
// Table decode: the four 8-bit offset tables of k_einsum_smallk_tbl are built
// as the kernel builds them from G_tbl's out map; their sum must equal the
// shift/mask decode and the mixed-radix loop.
// After the passing checks one shift, one mask and one table entry are
// perturbed and the same checks must then fail: the check can fail.
// plan_gather_kernel: kernel, grid and encoding at every threshold.
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

typedef std::vector<AxisInfo> Axes;

static u64 g_seed = 0x9e3779b97f4a7c15ull;
static u64 rnd() {  // 64-bit LCG: the same on every machine
  g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
  return g_seed >> 33;
}

static u64 elems_of(const Axes& ax) {
  u64 n = 1;
  for (const AxisInfo& a : ax) n *= a.dim;
  return n;
}

// ---- the decodes ----------------------------------------------------------

// the kernels' decode (gather2<P2>), encoding taken from the map
static void decode(const GatherMap& m, u64 p, i64* oa, i64* ob) {
  i64 a = 0, b = 0;
  for (int i = 0; i < m.n; ++i) {
    u64 c = m.pow2 ? ((p >> m.pstride[i]) & m.dim[i])
                   : ((p / m.pstride[i]) % m.dim[i]);
    a += (i64)c * m.sa[i];
    b += (i64)c * m.sb[i];
  }
  *oa = a;
  *ob = b;
}

// the reference: peel coordinates off p, innermost axis first
static void mixed_radix(const Axes& ax, u64 p, i64* oa, i64* ob) {
  i64 a = 0, b = 0;
  for (int i = (int)ax.size() - 1; i >= 0; --i) {
    const u64 c = p % ax[i].dim;
    p /= ax[i].dim;
    a += (i64)c * ax[i].sa;
    b += (i64)c * ax[i].sb;
  }
  *oa = a;
  *ob = b;
}

static bool map_agrees(const Axes& ax, const GatherMap& m, u64 p) {
  i64 oa, ob, ra, rb;
  decode(m, p, &oa, &ob);
  mixed_radix(ax, p, &ra, &rb);
  return oa == ra && ob == rb;
}

// every packed index of the list (a seeded sample of 2^16 past 2^20 elements)
static bool map_ok(const Axes& ax, const GatherMap& m) {
  if (m.n != (int)ax.size()) return false;
  const u64 n = elems_of(ax);
  if (n <= (1ull << 20)) {
    for (u64 p = 0; p < n; ++p)
      if (!map_agrees(ax, m, p)) return false;
    return true;
  }
  for (int x = 0; x < (1 << 16); ++x)
    if (!map_agrees(ax, m, ((rnd() << 31) ^ rnd()) % n)) return false;
  return map_agrees(ax, m, n - 1);
}

// both encodings of one axis list; returns whether the list is pow2
static bool check_axes(const Axes& ax) {
  GatherMap m;
  CHECK(build_map(ax, &m, false) == 0);
  CHECK(m.pow2 == 0);
  CHECK(map_ok(ax, m));
  CHECK(build_map(ax, &m, true) == 0);
  CHECK(m.pow2 == (axes_pow2(ax) ? 1 : 0));
  CHECK(map_ok(ax, m));
  CHECK(build_map(ax, &m) == 0);  // the default allows pow2
  CHECK(m.pow2 == (axes_pow2(ax) ? 1 : 0));
  return m.pow2 != 0;
}

// ---- the reach table's gather cases ---------------------------------------

struct Operand {
  std::vector<u64> labels, dims;
  std::vector<i64> strides;  // empty: contiguous row-major
};

static Meta meta_of(const Operand& t) {
  Meta m;
  m.nd = (int)t.labels.size();
  m.data = nullptr;
  i64 stride = 1;
  for (int x = m.nd - 1; x >= 0; --x) {
    m.labels[x] = t.labels[x];
    m.dims[x] = t.dims[x];
    m.strides[x] = t.strides.empty() ? stride : t.strides[x];
    stride *= (i64)t.dims[x];
  }
  return m;
}

struct Launch {
  Axes oax, kax;
  StepPlan p;
};

// the axis lists run_gather builds for the step, and the step's plan
static Launch launch_of(const Operand& a, const Operand& b,
                        const std::vector<u64>& out) {
  Launch L;
  const Meta A = meta_of(a), B = meta_of(b);
  std::vector<u64> shape;
  for (u64 lab : out) {
    u64 d = 0;
    for (size_t x = 0; x < a.labels.size(); ++x)
      if (a.labels[x] == lab) d = a.dims[x];
    for (size_t x = 0; x < b.labels.size(); ++x)
      if (b.labels[x] == lab) d = b.dims[x];
    CHECK(d);
    shape.push_back(d);
  }
  std::string err;
  CHECK(plan_step(true, out.data(), shape.data(), (int)out.size(), A, B,
                  false, &L.p, &err) == TN_OK);
  L.oax = gather_out_axis_info(L.p, shape.data(), (int)out.size(), A, B);
  L.kax = gather_k_axis_info(L.p, A, B);
  CHECK(elems_of(L.oax) == L.p.nout() && elems_of(L.kax) == L.p.k);
  return L;
}

// plan, both maps in the launch's encoding and in the other one
static Launch check_case(const Operand& a, const Operand& b,
                         const std::vector<u64>& out, int kernel,
                         int blocks) {
  Launch L = launch_of(a, b, out);
  CHECK(L.p.route == TN_ROUTE_GATHER);
  CHECK(L.p.gather_kernel == kernel && L.p.gather_blocks == blocks);
  const GatherChoice gc =
      plan_gather_kernel(L.oax, L.kax, L.p.nout(), L.p.k);
  CHECK(gc.kernel == kernel && gc.blocks == blocks);
  const bool o2 = check_axes(L.oax), k2 = check_axes(L.kax);
  CHECK(gc.pow2 == (o2 && k2));
  // the joint encoding: one non-pow2 map forces div/mod on the other
  GatherMap om, km;
  CHECK(build_map(L.oax, &om, gc.pow2) == 0);
  CHECK(build_map(L.kax, &km, gc.pow2) == 0);
  CHECK(om.pow2 == (gc.pow2 ? 1 : 0) && km.pow2 == om.pow2);
  return L;
}

static Operand qubits(const std::vector<u64>& labels) {
  return {labels, std::vector<u64>(labels.size(), 2), {}};
}

// ---- k_einsum_smallk_tbl --------------------------------------------------

struct Tables {
  i64 ta[4][256], tb[4][256];
};

// as the kernel fills them
static void build_tables(const GatherMap& omap, Tables* T) {
  for (int t = 0; t < 1024; ++t) {
    const int ti = t >> 8, e = t & 255;
    decode(omap, (u64)e << (8 * ti), &T->ta[ti][e], &T->tb[ti][e]);
  }
}

static bool table_agrees(const Axes& ax, const GatherMap& omap,
                         const Tables& T, u64 p) {
  const unsigned lo = (unsigned)p;
  const i64 oa = T.ta[0][lo & 255] + T.ta[1][(lo >> 8) & 255] +
                 T.ta[2][(lo >> 16) & 255] + T.ta[3][lo >> 24];
  const i64 ob = T.tb[0][lo & 255] + T.tb[1][(lo >> 8) & 255] +
                 T.tb[2][(lo >> 16) & 255] + T.tb[3][lo >> 24];
  i64 da, db, ra, rb;
  decode(omap, p, &da, &db);
  mixed_radix(ax, p, &ra, &rb);
  return oa == da && ob == db && oa == ra && ob == rb;
}

// every p below 2^16, every p with a single byte set, 2^20 seeded p
static bool tables_ok(const Axes& ax, const GatherMap& omap, const Tables& T,
                      u64 nout, u64 seed) {
  for (u64 p = 0; p < (1ull << 16) && p < nout; ++p)
    if (!table_agrees(ax, omap, T, p)) return false;
  for (int byte = 0; byte < 4; ++byte)
    for (u64 v = 1; v < 256; ++v) {
      const u64 p = v << (8 * byte);
      if (p < nout && !table_agrees(ax, omap, T, p)) return false;
    }
  g_seed = seed;
  for (int x = 0; x < (1 << 20); ++x)
    if (!table_agrees(ax, omap, T, ((rnd() << 31) ^ rnd()) % nout))
      return false;
  return table_agrees(ax, omap, T, nout - 1);
}

// ---- plan_gather_kernel at its thresholds ---------------------------------

static Axes pow2_axes(int n, int first_log2 = 1) {
  Axes ax;
  for (int i = 0; i < n; ++i)
    ax.push_back({i == 0 ? (1ull << first_log2) : 2ull, 1, 0});
  return ax;
}

static void expect(const Axes& oax, const Axes& kax, u64 nout, u64 K,
                   int kernel, int blocks, bool pow2) {
  const GatherChoice gc = plan_gather_kernel(oax, kax, nout, K);
  if (gc.kernel != kernel || gc.blocks != blocks || gc.pow2 != pow2) {
    fprintf(stderr,
            "plan_gather_kernel(n=%zu, nout=%llu, K=%llu): kernel %d blocks "
            "%d pow2 %d, expected %d %d %d\n",
            oax.size(), (unsigned long long)nout, (unsigned long long)K,
            gc.kernel, gc.blocks, (int)gc.pow2, kernel, blocks, (int)pow2);
    exit(1);
  }
}

static void check_thresholds() {
  const int cap = 64 * 2048, tcap = 32768;
  const Axes o8 = pow2_axes(8, 19), o7 = pow2_axes(7, 20), k4 = pow2_axes(2);
  const Axes k64 = pow2_axes(1, 6);
  const u64 b26 = 1ull << 26, b32 = 1ull << 32;
  // the table kernel's window: 2^26 <= nout < 2^32, rank >= 8
  expect(o8, k4, b26 - 1, 4, TN_GK_SMALLK_P2, cap, true);
  expect(o8, k4, b26, 4, TN_GK_SMALLK_TBL, tcap, true);
  expect(o8, k4, b32 - 1, 4, TN_GK_SMALLK_TBL, tcap, true);
  expect(o8, k4, b32, 4, TN_GK_SMALLK_P2, cap, true);
  expect(o7, k4, b26, 4, TN_GK_SMALLK_P2, cap, true);
  // K = TN_SMALLK is the last smallk shape
  expect(o8, k64, b26, 64, TN_GK_SMALLK_TBL, tcap, true);
  expect(o8, k64, b26, 65, TN_GK_ANYK_P2, cap, true);
  expect(o7, k64, 1 << 10, 64, TN_GK_SMALLK_P2, 4, true);
  expect(o7, k64, 1 << 10, 65, TN_GK_ANYK_P2, 4, true);
  // one non-pow2 axis in either map: div/mod for both
  Axes o8x = o8, k3 = {{3, 1, 1}};
  o8x[5].dim = 6;
  expect(o8x, k4, b26, 4, TN_GK_SMALLK, cap, false);
  expect(o8, k3, b26, 3, TN_GK_SMALLK, cap, false);
  expect(o8x, k64, b26, 65, TN_GK_ANYK, cap, false);
  expect(o8, k3, b26, 65, TN_GK_ANYK, cap, false);
  // the grid: one block per 256 elements, at least one, capped
  expect(Axes(), k4, 1, 4, TN_GK_SMALLK_P2, 1, true);
  expect(o7, k4, 256, 4, TN_GK_SMALLK_P2, 1, true);
  expect(o7, k4, 257, 4, TN_GK_SMALLK_P2, 2, true);
  expect(o7, k4, (u64)cap * 256, 4, TN_GK_SMALLK_P2, cap, true);
  expect(o7, k4, (u64)cap * 256 + 1, 4, TN_GK_SMALLK_P2, cap, true);
  expect(o7, k4, (u64)(cap - 1) * 256 + 1, 4, TN_GK_SMALLK_P2, cap, true);
  expect(o7, k4, (u64)(cap - 1) * 256, 4, TN_GK_SMALLK_P2, cap - 1, true);
}

int main() {
  // ---- the table's cases: plan and maps
  check_case({{1, 2, 101}, {3, 5, 7}, {}}, {{101, 201}, {7, 4}, {}},
             {1, 2, 201}, TN_GK_SMALLK, 1);  // G_np2
  const Operand q8 = qubits({1, 2, 3, 101, 4, 102, 5, 6});
  const Operand gate = qubits({201, 202, 101, 102});
  check_case(q8, gate, {1, 2, 3, 201, 4, 202, 5, 6}, TN_GK_SMALLK_P2,
             1);  // G_gate
  check_case(q8, gate, {4, 202, 1, 6, 201, 2, 3, 5}, TN_GK_SMALLK_P2,
             1);  // G_gate_outorder
  check_case({{1, 101}, {8, 64}, {}}, {{101, 201}, {64, 300}, {}}, {1, 201},
             TN_GK_SMALLK, 10);  // G_k64
  check_case({{1, 101}, {100, 64}, {}}, {{101, 201}, {64, 50}, {}}, {1, 201},
             TN_GK_SMALLK, 20);  // G_k64_mid
  check_case({{1, 101}, {8, 65}, {}}, {{101, 201}, {65, 300}, {}}, {1, 201},
             TN_GK_ANYK, 10);  // G_k65
  check_case({{1, 101, 102}, {3, 5, 13}, {}},
             {{102, 101, 201}, {13, 5, 301}, {}}, {1, 201}, TN_GK_ANYK,
             4);  // G_k65_np2
  check_case({{1, 101}, {4, 1024}, {}}, {{101, 201}, {1024, 4096}, {}},
             {1, 201}, TN_GK_ANYK_P2, 64);  // G_anyk_p2
  check_case({{101}, {64}, {}}, {{101, 201}, {64, 1000}, {}}, {201},
             TN_GK_SMALLK, 4);  // G_m1
  {
    Launch L = check_case({{101}, {64}, {}}, {{101}, {64}, {}}, {},
                          TN_GK_SMALLK_P2, 1);  // G_scalar64
    CHECK(L.oax.empty());
    // one more K element is a dot, with no gather kernel
    const Operand v65 = {{101}, {65}, {}};
    const Meta A = meta_of(v65), B = meta_of(v65);
    StepPlan p;
    std::string err;
    CHECK(plan_step(true, nullptr, nullptr, 0, A, B, false, &p, &err) ==
          TN_OK);
    CHECK(p.route == TN_ROUTE_DOT && p.dot_form == TN_DOT_LINEAR);
    CHECK(p.gather_kernel == TN_GK_NONE && p.gather_blocks == 0);
  }
  {
    Launch L = check_case({{1}, {5}, {}}, {{201}, {6}, {}}, {1, 201},
                          TN_GK_SMALLK, 1);  // G_outer
    CHECK(L.kax.size() == 1 && L.kax[0].dim == 1);
  }
  {
    Launch L = check_case({{1, 101}, {3, 2}, {8, 1}},
                          {{101, 201}, {2, 5}, {}}, {1, 201}, TN_GK_SMALLK,
                          1);  // G_strided
    CHECK(L.oax[0].sa == 8 && L.kax[0].sa == 1 && L.kax[0].sb == 5);
  }
  check_case({{1}, {8209}, {}}, {{201}, {4099}, {}}, {1, 201}, TN_GK_SMALLK,
             64 * 2048);  // G_pass2_np2
  check_case({{1}, {8192}, {}}, {{201}, {8192}, {}}, {1, 201},
             TN_GK_SMALLK_P2, 64 * 2048);  // G_pass2_p2

  // ---- G_tbl: 26 qubits, the gate's at positions 3 and 17
  std::vector<u64> q26;
  for (u64 l = 1; l <= 24; ++l) {
    if (q26.size() == 3) q26.push_back(101);
    if (q26.size() == 17) q26.push_back(102);
    q26.push_back(l);
  }
  CHECK(q26.size() == 26 && q26[3] == 101 && q26[17] == 102);
  const std::vector<u64> out26 = {15, 21, 2,  4,  6,  10, 7,  202, 8,
                                  11, 22, 16, 13, 19, 24, 9,  1,   201,
                                  3,  14, 17, 20, 23, 12, 18, 5};
  const Launch tbl =
      check_case(qubits(q26), gate, out26, TN_GK_SMALLK_TBL, 32768);
  const u64 nout = tbl.p.nout();
  CHECK(nout == (1ull << 26) && tbl.oax.size() == 26);
  GatherMap omap;
  CHECK(build_map(tbl.oax, &omap, true) == 0 && omap.pow2 == 1);
  Tables* T = new Tables;
  build_tables(omap, T);
  CHECK(tables_ok(tbl.oax, omap, *T, nout, 26));
  // bits 24 and 25 of the index come from table 3 and carry an offset
  CHECK(T->ta[3][1] + T->tb[3][1] != 0 && T->ta[3][2] + T->tb[3][2] != 0);

  // ---- self-tests: the checks can fail
  {
    GatherMap bad = omap;
    bad.pstride[7] += 1;  // a shift
    CHECK(!map_ok(tbl.oax, bad));
    bad = omap;
    bad.dim[11] = 3;  // a mask
    CHECK(!map_ok(tbl.oax, bad));
    Tables* B = new Tables(*T);
    B->ta[2][17] += 1;  // a table entry
    CHECK(!tables_ok(tbl.oax, omap, *B, nout, 26));
    *B = *T;
    B->tb[3][2] += 1;  // reached by bit 25 alone
    CHECK(!tables_ok(tbl.oax, omap, *B, nout, 26));
    delete B;
    // tables built from a perturbed map disagree with the mixed-radix loop
    bad = omap;
    std::swap(bad.pstride[0], bad.pstride[1]);
    B = new Tables;
    build_tables(bad, B);
    CHECK(!tables_ok(tbl.oax, bad, *B, nout, 26));
    delete B;
    // div/mod: a packed stride
    const Axes np2 = {{3, 20, 0}, {5, 4, 0}, {4, 0, 1}};
    GatherMap dm;
    CHECK(build_map(np2, &dm, true) == 0 && dm.pow2 == 0 && map_ok(np2, dm));
    dm.pstride[0] -= 1;
    CHECK(!map_ok(np2, dm));
    CHECK(build_map(np2, &dm, true) == 0);
    dm.dim[1] = 4;
    CHECK(!map_ok(np2, dm));
  }
  delete T;

  // ---- seeded random axis lists: rank 0..12, dims 1..8, strides with gaps
  g_seed = 12;
  int npow2 = 0, nnot = 0;
  for (int trial = 0; trial < 400; ++trial) {
    const int rank = (int)(rnd() % 13);
    const bool want_pow2 = trial & 1;
    Axes ax(rank);
    i64 sa = 1, sb = 1;
    u64 total = 1;
    for (int i = rank - 1; i >= 0; --i) {
      u64 d = want_pow2 ? (1ull << (rnd() % 4)) : 1 + rnd() % 8;
      if (total * d > (1ull << 16)) d = 1;
      total *= d;
      // an axis lives in A, in B or (a batch axis) in both
      const int where = (int)(rnd() % 3);
      sa *= 1 + (i64)(rnd() % 3);  // gaps
      sb *= 1 + (i64)(rnd() % 2);
      ax[i] = {d, where != 1 ? sa : 0, where != 0 ? sb : 0};
      sa *= (i64)d;
      sb *= (i64)d;
    }
    (check_axes(ax) ? npow2 : nnot) += 1;
  }
  CHECK(npow2 >= 100 && nnot >= 100);

  // ---- rank
  GatherMap m;
  CHECK(build_map(Axes(TN_MAXR, AxisInfo{1, 0, 0}), &m) == 0);
  CHECK(build_map(Axes(TN_MAXR + 1, AxisInfo{1, 0, 0}), &m) == -1);

  check_thresholds();
  printf("gather_map_check OK\n");
  return 0;
}
