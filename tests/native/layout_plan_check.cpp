// Stand-alone host check of the scatter-epilogue gate (plan_step) and the
// walk plan (plan_layouts: stored orders, look-ahead packs, inline pack
// bytes). Needs only a host compiler, e.g.
//   g++ -std=c++17 -O1 -g -Wall -fsanitize=address,undefined
//       -fno-sanitize-recover=undefined tests/native/layout_plan_check.cpp
// Exit 0 and "layout_plan_check OK" on success. With TN_EPI_SCATTER=0 in the
// environment it checks the switched-off behaviour instead.
//
// Besides the route cases of tests/test_layout_plan.py it replays, on the
// host, the address arithmetic of the scatter epilogue (tile-origin part +
// 128-entry row table + 64-entry column table) for every element of each
// admitted case and checks it against the element's row-major offset in out
// order: every store in bounds, every destination hit exactly once.
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

static Legs sub(const Legs& v, size_t a, size_t b) {
  return Legs(v.begin() + a, v.begin() + b);
}

struct Case {
  LayoutTensor out, a, b;
};

static LayoutTensor tensor(const Legs& l, u64 wide_label = 0, u64 wide = 2) {
  LayoutTensor t;
  t.labels = l;
  for (u64 lab : l) t.dims.push_back(lab == wide_label ? wide : 2);
  return t;
}

static Case mk(const Legs& out, const Legs& m, const Legs& n, const Legs& k,
               u64 wide_label = 0, u64 wide = 2) {
  return {tensor(out, wide_label, wide), tensor(cat({m, k}), wide_label, wide),
          tensor(cat({k, n}), wide_label, wide)};
}

static StepPlan plan(const Case& c) {
  StepPlan p;
  CHECK(layout_plan_step(true, c.out, c.a, c.b, true, &p));
  return p;
}

// the scatter epilogue's addressing, as k_zgemm_c128_glds_3m_scatter forms it
static void check_scatter_addresses(const Case& c, const StepPlan& p) {
  const ScatterMap& sm = p.smap;
  CHECK((1ull << sm.rbits) == p.m && (1ull << sm.cbits) == p.n);
  CHECK(sm.rbits >= 7 && sm.cbits >= 6);
  std::vector<u64> rowtab(MF_T), coltab(MF_TN);
  for (int t = 0; t < MF_T; ++t)
    for (int b = 0; b < 7; ++b)
      if ((t >> b) & 1) rowtab[t] += sm.rstride[b];
  for (int t = 0; t < MF_TN; ++t)
    for (int b = 0; b < 6; ++b)
      if ((t >> b) & 1) coltab[t] += sm.cstride[b];
  // reference: decode row / col into leg indices, offset in out order
  const int nd = (int)c.out.labels.size();
  std::vector<u64> ostride(nd);
  u64 stride = 1;
  for (int i = nd - 1; i >= 0; --i) {
    ostride[i] = stride;
    stride *= c.out.dims[i];
  }
  auto ref_part = [&](u64 idx, const AxisList& axes) {
    u64 off = 0;
    for (int t = axes.n - 1; t >= 0; --t) {
      const u64 d = c.out.dims[axes[t]];
      off += (idx % d) * ostride[axes[t]];
      idx /= d;
    }
    return off;
  };
  const u64 nout = p.m * p.n;
  std::vector<u64> rref(p.m), cref(p.n);
  for (u64 r = 0; r < p.m; ++r) rref[r] = ref_part(r, p.m_out);
  for (u64 q = 0; q < p.n; ++q) cref[q] = ref_part(q, p.n_out);
  std::vector<unsigned char> hit(nout, 0);
  for (u64 brow = 0; brow < p.m; brow += MF_T)
    for (u64 bcol = 0; bcol < p.n; bcol += MF_TN) {
      u64 base = 0;
      for (int b = 7; b < sm.rbits; ++b)
        if ((brow >> b) & 1) base += sm.rstride[b];
      for (int b = 6; b < sm.cbits; ++b)
        if ((bcol >> b) & 1) base += sm.cstride[b];
      for (int r = 0; r < MF_T; ++r)
        for (int q = 0; q < MF_TN; ++q) {
          const u64 off = base + rowtab[r] + coltab[q];
          CHECK(off < nout);
          CHECK(off == rref[brow + r] + cref[bcol + q]);
          CHECK(!hit[off]);
          hit[off] = 1;
        }
    }
}

int main() {
  const bool on = env_switch(ENV_EPI_SCATTER) != 0;
  const Legs M = legs(100, 11), N = legs(200, 10), K = legs(300, 5);
  const Legs inter = cat({sub(M, 0, 6), sub(N, 0, 4), sub(M, 6, 10),
                          sub(N, 4, 7), sub(M, 10, 11), sub(N, 7, 10)});
  const Legs run2 = cat({sub(M, 0, 6), sub(N, 0, 4), sub(M, 6, 10),
                         sub(N, 4, 8), sub(M, 10, 11), sub(N, 8, 10)});
  const Legs mlow = cat({sub(N, 0, 5), sub(M, 0, 10), sub(N, 5, 10),
                         sub(M, 10, 11)});
  const Legs merged = cat({sub(M, 0, 6), sub(N, 0, 4), sub(M, 6, 11),
                           sub(N, 4, 9)});
  // the seven tile-local row bits on top of everything: destination bits
  // 14..20 here, and 21..27 with N = 2^17 (byte offsets up to 2^32)
  const Legs rows_high = cat({sub(M, 4, 11), sub(N, 0, 7), sub(M, 0, 4),
                              sub(N, 7, 10)});
  const Legs N17 = legs(200, 17);
  const Legs rows_high17 = cat({sub(M, 4, 11), sub(N17, 0, 14), sub(M, 0, 4),
                                sub(N17, 14, 17)});

  struct {
    const char* name;
    Case c;
    bool scatter;
  } cases[] = {
      {"interleaved", mk(inter, M, N, K), true},
      {"run2", mk(run2, M, N, K), false},
      {"m_lowest", mk(mlow, M, N, K), false},
      {"dim4", mk(merged, M, sub(N, 0, 9), K, 208, 4), true},
      {"dim3", mk(merged, M, sub(N, 0, 9), K, 208, 3), false},
      {"k16", mk(inter, M, N, sub(K, 0, 4)), false},
      {"tiles128",
       mk(Legs(inter.begin() + 1, inter.end()), sub(M, 1, 11), N, K), false},
      {"rows_high", mk(rows_high, M, N, K), true},
      {"rows_high17", mk(rows_high17, M, N17, K), true},
  };
  for (auto& t : cases) {
    const StepPlan p = plan(t.c);
    const bool expect = t.scatter && on;
    if (p.scatter_out != (expect ? 1 : 0)) {
      fprintf(stderr, "%s: scatter_out %d, expected %d\n", t.name,
              p.scatter_out, (int)expect);
      return 1;
    }
    CHECK(!p.direct);
    CHECK(p.kind == (expect ? 2 : 3));
    CHECK(p.ws_tmp_c == (expect ? 0 : p.m * p.n * 16));
    if (expect) check_scatter_addresses(t.c, p);
  }
  // c64 never scatters
  {
    StepPlan p;
    const Case c = mk(inter, M, N, K);
    CHECK(layout_plan_step(false, c.out, c.a, c.b, true, &p));
    CHECK(!p.scatter_out && p.kind == 3);
  }

  // pre-pass on a three-leaf chain: step 0 = the gated shape, step 1
  // contracts six legs of M_0 and four of N_0 against leaf 2
  {
    const Legs k1 = cat({sub(M, 5, 11), sub(N, 6, 10)});
    std::vector<LayoutTensor> leaves = {
        tensor(cat({M, K})), tensor(cat({K, N})),
        tensor(cat({k1, legs(400, 6)}))};
    const u64 pairs[] = {0, 1, 0, 2};
    LayoutPlan lp;
    plan_layouts(true, leaves, pairs, 2, &lp);
    CHECK(lp.valid && lp.out.size() == 2);
    CHECK(lp.scatter_out[0] == (on ? 1 : 0) && lp.scatter_out[1] == 0);
    // M_1 = M[0:5] + N[0:6]: 2^11 rows, K_1 = 2^10
    CHECK(lp.inline_pack_bytes[1] == (on ? 0 : (1ull << 21) * 16));
    const Legs stored0 =
        on ? cat({sub(M, 0, 5), sub(N, 0, 6), sub(M, 5, 11), sub(N, 6, 10)})
           : cat({M, N});
    CHECK(lp.out[0].labels == stored0);
    // the last step keeps the symmetric-difference order of today's walk
    CHECK(lp.out[1].labels == cat({sub(M, 0, 5), sub(N, 0, 6), legs(400, 6)}));
    // c64, and an invalid path
    plan_layouts(false, leaves, pairs, 2, &lp);
    CHECK(lp.valid && !lp.scatter_out[0] && lp.out[0].labels == cat({M, N}));
    const u64 bad[] = {0, 1, 1, 2};
    plan_layouts(true, leaves, bad, 2, &lp);
    CHECK(!lp.valid);
  }

  // walk plan of a four-leaf network whose three steps are all TTGT:
  //   0 = M+K, 1 = K+N, 2 = X+K1, 3 = K2+Y      path (0,1) (0,2) (3,0)
  // 2048x1024x32, then 2048x64x1024 against leaf 2, then 128x64x2048 with
  // leaf 3 as A. Step 1 can pack only its B early (step 0 makes its A),
  // step 2 only its A (step 1 makes its B).
  {
    const Legs X = legs(400, 6), Y = legs(500, 7);
    const Legs k1 = cat({sub(M, 5, 11), sub(N, 6, 10)});
    const Legs k2 = cat({X, sub(N, 0, 5)});
    std::vector<LayoutTensor> leaves = {
        tensor(cat({M, K})), tensor(cat({K, N})), tensor(cat({X, k1})),
        tensor(cat({k2, Y}))};
    const u64 pairs[] = {0, 1, 0, 2, 3, 0};
    LayoutPlan lp;
    plan_layouts(true, leaves, pairs, 3, &lp);
    CHECK(lp.valid && lp.out.size() == 3 && lp.early.size() == 3);
    const Legs rows1 = cat({sub(M, 0, 5), sub(N, 0, 6)});
    CHECK(lp.out[0].labels == (on ? cat({rows1, k1}) : cat({M, N})));
    CHECK(lp.out[1].labels == cat({rows1, X}));
    CHECK(lp.out[2].labels == cat({Y, sub(M, 0, 5), sub(N, 5, 6)}));
    CHECK(lp.scatter_out == std::vector<int32_t>({on ? 1 : 0, 0, 0}));
    // look-ahead packs: the same with the scatter epilogue on and off
    const EarlyPack &e0 = lp.early[0], &e1 = lp.early[1], &e2 = lp.early[2];
    CHECK(!e0.a && !e0.b);
    CHECK(!e1.a && e1.b && e1.a_elems == 0 && e1.b_elems == (1ull << 16));
    std::vector<int> k1_then_x, y_then_k2;  // leaf 2 as [K1][X], 3 as [Y][K2]
    for (int x = 0; x < 16; ++x) k1_then_x.push_back((x + 6) % 16);
    for (int x = 0; x < 18; ++x) y_then_k2.push_back((x + 11) % 18);
    CHECK(e1.a_axes.empty() && e1.b_axes == k1_then_x);
    CHECK(e2.a && !e2.b && e2.a_elems == (1ull << 18) && e2.b_elems == 0);
    CHECK(e2.a_axes == y_then_k2 && e2.b_axes.empty());
    // inline: step 1's A only when step 0 stored the plain order, step 2's B
    CHECK(lp.inline_pack_bytes ==
          std::vector<u64>({0, on ? 0 : (1ull << 21) * 16, (1ull << 17) * 16}));
    // no plan: a dead operand, and a leaf of rank 41
    const u64 bad[] = {0, 1, 1, 2, 3, 0};
    plan_layouts(true, leaves, bad, 3, &lp);
    CHECK(!lp.valid && lp.err == "invalid contraction path step");
    CHECK(lp.out.empty() && lp.early.empty());
    leaves[3] = tensor(legs(600, 41));
    plan_layouts(true, leaves, pairs, 3, &lp);
    CHECK(!lp.valid && lp.err == "tensor rank exceeds 40");
  }
  printf("layout_plan_check OK (scatter %s)\n", on ? "on" : "off");
  return 0;
}
