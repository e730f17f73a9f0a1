// Stand-alone host check of the sampling plan and pick rules (plan_sample,
// sample_pick_chunk, sample_pick_in_chunk: step_plan.hpp). Needs only a host
// compiler, e.g.
//   g++ -std=c++17 -O1 -g -Wall -fsanitize=address,undefined
//       -fno-sanitize-recover=undefined tests/native/sample_plan_check.cpp
// Exit 0 and "sample_plan_check OK" on success.
//
// The pick functions are what k_sample_draw restates. Here they run against
// brute-force loops that state the rule directly (first prefix value above t
// in a plain left-to-right sum, else the last entry that added mass) on
// integer and dyadic masses, where every partial sum is exact and the order of
// the adds cannot matter. The self-tests at the end run the same cases through
// variants with > turned into >= and must see them fail.
#include <cmath>
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

typedef u64 (*PickChunk)(const double*, u64, double);
typedef u64 (*PickIn)(const double*, u64, double);

// ---- the rules, stated directly -------------------------------------------

static u64 brute_chunk(const double* C, u64 nchunks, double t) {
  for (u64 j = 0; j < nchunks; ++j)
    if (C[j] > t) return j;
  for (u64 j = nchunks; j-- > 0;)
    if (C[j] > (j ? C[j - 1] : 0.0)) return j;
  return 0;
}

static u64 brute_in_chunk(const double* p, u64 len, double t) {
  double r = 0.0;
  for (u64 i = 0; i < len; ++i) {
    r += p[i];
    if (r > t) return i;
  }
  for (u64 i = len; i-- > 0;)
    if (p[i] > 0.0) return i;
  return 0;
}

// ---- the >= variants the self-tests must catch ----------------------------

static u64 ge_chunk(const double* C, u64 nchunks, double t) {
  for (u64 j = 0; j < nchunks; ++j)
    if (C[j] >= t) return j;
  return brute_chunk(C, nchunks, t);
}

static u64 ge_in_chunk(const double* p, u64 len, double t) {
  double r = 0.0;
  for (u64 i = 0; i < len; ++i) {
    r += p[i];
    if (p[i] > 0.0 && r >= t) return i;
  }
  return brute_in_chunk(p, len, t);
}

// ---- plan -----------------------------------------------------------------

static void check_plan() {
  struct Case {
    u64 n, nchunks;
  } cases[] = {{1, 1},       {4095, 1},
               {4096, 1},    {4097, 2},
               {1ull << 34, 1ull << 22}};
  const u64 shots[] = {0, 1, 1000, 1000000};
  for (const Case& c : cases)
    for (u64 esize : {16, 8})
      for (u64 ns : shots) {
        SamplePlan sp;
        plan_sample(c.n, ns, esize, &sp);
        CHECK(sp.valid && sp.err.empty());
        CHECK(sp.chunk == 4096 && sp.chunk == TN_SAMPLE_CHUNK);
        CHECK(sp.nchunks == c.nchunks);
        CHECK(sp.grid_sums == c.nchunks && sp.grid_scan == 1);
        CHECK(sp.grid_draw == ns);
        CHECK(sp.off_u == 8 * c.nchunks);
        CHECK(sp.off_idx == sp.off_u + 8 * ns);
        CHECK(sp.off_total == sp.off_idx + 8 * ns);
        CHECK(sp.ws_bytes == 8 * c.nchunks + 16 * ns + 8);
      }
  SamplePlan sp;
  plan_sample(0, 5, 16, &sp);
  CHECK(!sp.valid && sp.err == "tensor has no elements");
  plan_sample(4096, 5, 4, &sp);
  CHECK(!sp.valid && !sp.err.empty());
  plan_sample(4096, 1ull << 31, 16, &sp);
  CHECK(!sp.valid && sp.err == "more chunks or shots than one grid holds");
  plan_sample(~(u64)0, 1, 16, &sp);
  CHECK(!sp.valid && sp.err == "tensor size overflows 64 bits");
  plan_sample((1ull << 31) * 4096, 1, 8, &sp);
  CHECK(!sp.valid);  // 2^31 chunks
}

// ---- the arrays -----------------------------------------------------------

static std::vector<double> prefix(const std::vector<double>& S) {
  std::vector<double> C(S.size());
  double run = 0.0;
  for (size_t j = 0; j < S.size(); ++j) C[j] = run += S[j];
  return C;
}

// the values of t worth asking at: 0, every prefix value, one ulp to either
// side of it, halfway into every entry, total and beyond
static std::vector<double> probes(const std::vector<double>& C) {
  std::vector<double> ts = {0.0};
  double prev = 0.0;
  for (double c : C) {
    ts.push_back(c);
    ts.push_back(std::nextafter(c, 0.0));
    ts.push_back(std::nextafter(c, INFINITY));
    ts.push_back(prev + (c - prev) / 2);
    prev = c;
  }
  const double total = C.empty() ? 0.0 : C.back();
  ts.push_back(total * 2 + 1);
  ts.push_back(INFINITY);
  return ts;
}

// masses with zeros at the front, at the back and around slab and chunk
// boundaries; integers, or integers times 2^-20
static std::vector<std::vector<double>> mass_arrays(u64 len) {
  std::vector<std::vector<double>> out;
  auto blank = [&] { return std::vector<double>(len, 0.0); };
  {  // all mass in the last element
    auto p = blank();
    p[len - 1] = 5;
    out.push_back(p);
  }
  {  // all mass in the first element
    auto p = blank();
    p[0] = 3;
    out.push_back(p);
  }
  {  // every element, small integers with a third of them zero
    auto p = blank();
    for (u64 i = 0; i < len; ++i) p[i] = (i * 7 + 3) % 3 ? (i * 5) % 9 : 0;
    out.push_back(p);
  }
  {  // zeros in front, behind, and on both sides of every 16th / 4096th
    auto p = blank();
    for (u64 i = 0; i < len; ++i) {
      const u64 m = i % TN_SAMPLE_SLAB;
      p[i] = (m == 0 || m == TN_SAMPLE_SLAB - 1 || i < 40 || i + 40 >= len)
                 ? 0.0
                 : (double)(1 + i % 4) / 1048576.0;
    }
    out.push_back(p);
  }
  {  // mass only next to the slab boundaries
    auto p = blank();
    for (u64 i = 0; i < len; ++i) {
      const u64 m = i % TN_SAMPLE_SLAB;
      p[i] = (m == 0 || m == TN_SAMPLE_SLAB - 1) ? 2.0 : 0.0;
    }
    out.push_back(p);
  }
  return out;
}

static int run_in_chunk(PickIn pick, bool stop_at_first) {
  int bad = 0;
  for (u64 len : {1ull, 2ull, 15ull, 16ull, 17ull, 63ull, 4095ull, 4096ull})
    for (const auto& p : mass_arrays(len)) {
      const auto C = prefix(p);
      for (double t : probes(C)) {
        const u64 want = brute_in_chunk(p.data(), len, t);
        const u64 got = pick(p.data(), len, t);
        CHECK(got < len);
        if (got != want) {
          if (stop_at_first) return 1;
          ++bad;
        } else if (C.back() > 0) {
          CHECK(p[got] > 0.0);  // an element without mass is never drawn
        }
      }
    }
  return bad;
}

static int run_chunk(PickChunk pick, bool stop_at_first) {
  int bad = 0;
  for (u64 len : {1ull, 2ull, 3ull, 17ull, 2049ull})
    for (const auto& S : mass_arrays(len)) {
      const auto C = prefix(S);
      for (double t : probes(C)) {
        const u64 want = brute_chunk(C.data(), len, t);
        const u64 got = pick(C.data(), len, t);
        CHECK(got < len);
        if (got != want) {
          if (stop_at_first) return 1;
          ++bad;
        } else if (C.back() > 0) {
          CHECK(S[got] > 0.0);  // a chunk without mass is never drawn
        }
      }
    }
  return bad;
}

// the two levels together draw what one plain scan over all elements draws
static void check_two_levels() {
  const u64 n = 3 * TN_SAMPLE_CHUNK + 5;
  std::vector<double> p(n);
  for (u64 i = 0; i < n; ++i) p[i] = (i * 11 + 1) % 3 ? (i * 13) % 50 : 0;
  // zeros around the chunk boundaries
  for (u64 b = TN_SAMPLE_CHUNK; b < n; b += TN_SAMPLE_CHUNK)
    for (u64 i = b - 3; i < b + 3; ++i) p[i] = 0;
  const u64 nchunks = (n - 1) / TN_SAMPLE_CHUNK + 1;
  std::vector<double> S(nchunks, 0.0);
  for (u64 i = 0; i < n; ++i) S[i / TN_SAMPLE_CHUNK] += p[i];
  const auto C = prefix(S);
  const auto all = prefix(p);
  std::vector<double> ts = probes(C);
  for (u64 i = 0; i < n; i += 97) {
    ts.push_back(all[i]);
    ts.push_back(std::nextafter(all[i], 0.0));
  }
  for (double t : ts) {
    const u64 j = sample_pick_chunk(C.data(), nchunks, t);
    const u64 base = j * TN_SAMPLE_CHUNK;
    const u64 len = std::min<u64>(TN_SAMPLE_CHUNK, n - base);
    const u64 i = base + sample_pick_in_chunk(p.data() + base, len,
                                              t - (j ? C[j - 1] : 0.0));
    const u64 want = brute_in_chunk(p.data(), n, t);
    CHECK(i == want);
    CHECK(p[i] > 0.0);
  }
}

// 2^21 chunks: the flat index of a draw in the upper half exceeds 2^32
static void check_large() {
  const u64 nchunks = 1ull << 21;
  std::vector<double> C(nchunks);
  for (u64 j = 0; j < nchunks; ++j) C[j] = (double)(3 * (j + 1));
  const u64 probe[] = {0, 1, (1ull << 20) - 1, 1ull << 20, (1ull << 20) + 1,
                       nchunks - 2, nchunks - 1};
  for (u64 j : probe) {
    CHECK(sample_pick_chunk(C.data(), nchunks, C[j]) ==
          (j + 1 < nchunks ? j + 1 : j));
    CHECK(sample_pick_chunk(C.data(), nchunks, C[j] - 1) == j);
    CHECK(sample_pick_chunk(C.data(), nchunks, C[j] - 3) == j);
  }
  const u64 j = sample_pick_chunk(C.data(), nchunks, C[nchunks - 5] - 1);
  const u64 flat = j * TN_SAMPLE_CHUNK + 4095;
  CHECK(j == nchunks - 5 && flat > (1ull << 32) && flat / TN_SAMPLE_CHUNK == j);
  // the clamp over a long run of chunks without mass
  for (u64 x = nchunks / 2; x < nchunks; ++x) C[x] = C[nchunks / 2 - 1];
  CHECK(sample_pick_chunk(C.data(), nchunks, C.back()) == nchunks / 2 - 1);
  CHECK(sample_pick_chunk(C.data(), nchunks, INFINITY) == nchunks / 2 - 1);
}

// what the documented corner cases give
static void check_corners() {
  const double none[3] = {0, 0, 0};
  CHECK(sample_pick_chunk(none, 3, 0.0) == 0);
  CHECK(sample_pick_in_chunk(none, 3, 0.0) == 0);
  const double nan = std::nan("");
  const double C[3] = {1, 1, 4};
  CHECK(sample_pick_chunk(C, 3, nan) == 2);
  const double p[4] = {1, 0, 2, 0};
  CHECK(sample_pick_in_chunk(p, 4, nan) == 2);
  // a positive sum lost in the rounding of the prefix adds no mass
  const double big[3] = {1e300, 1e300, 1e300};
  CHECK(sample_pick_chunk(big, 3, 1e300) == 0);
}

int main() {
  check_plan();
  CHECK(run_in_chunk(sample_pick_in_chunk, false) == 0);
  CHECK(run_chunk(sample_pick_chunk, false) == 0);
  check_two_levels();
  check_large();
  check_corners();
  // self-tests: the brute force passes its own run, the >= variants do not
  CHECK(run_in_chunk(brute_in_chunk, false) == 0);
  CHECK(run_chunk(brute_chunk, false) == 0);
  CHECK(run_in_chunk(ge_in_chunk, true) == 1);
  CHECK(run_chunk(ge_chunk, true) == 1);
  printf("sample_plan_check OK\n");
  return 0;
}
