// Stand-alone host check of the slice plan (plan_slices, step_plan.hpp).
// Needs only a host compiler, e.g.
//   g++ -std=c++17 -O1 -g -Wall -fsanitize=address,undefined
//       -fno-sanitize-recover=undefined tests/native/slice_plan_check.cpp
// Exit 0 and "slice_plan_check OK" on success.
//
// For a mixed-radix case and a pow2 chain it replays, on the host, the
// addressing of k_slice_gather (digit decode, base offset, div/mod or
// shift/mask over the remaining dims) for every assignment and every element
// of every sliced leaf, and checks each source index against the row-major
// index of the fixed-label element: in bounds, and the element meant. The
// refusals are checked for their message and for leaving the plan invalid.
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

static LayoutTensor tensor(std::vector<u64> labels, std::vector<u64> dims) {
  LayoutTensor t;
  t.labels = labels;
  t.dims = dims;
  return t;
}

static bool has(const std::vector<u64>& v, u64 x) {
  return std::find(v.begin(), v.end(), x) != v.end();
}

// every (assignment, sliced leaf, element): the gather's source index is the
// row-major index of that element with the slice labels at their digits
static void check_gather(const std::vector<LayoutTensor>& leaves,
                         const SlicePlan& sp) {
  const size_t nl = sp.labels.size();
  for (u64 t = 0; t < sp.count; ++t) {
    std::vector<u64> digit(nl);
    for (size_t x = 0; x < nl; ++x)
      digit[x] = (t / sp.weights[x]) % sp.radices[x];
    // first label most significant
    u64 again = 0;
    for (size_t x = 0; x < nl; ++x) again = again * sp.radices[x] + digit[x];
    CHECK(again == t);
    for (size_t l = 0; l < leaves.size(); ++l) {
      const LayoutTensor& full = leaves[l];
      const LayoutTensor& red = sp.reduced[l];
      u64 full_elems = 1, red_elems = 1, base = 0;
      for (u64 d : full.dims) full_elems *= d;
      for (u64 d : red.dims) red_elems *= d;
      bool carries = false;
      for (size_t x = 0; x < nl; ++x) {
        CHECK((sp.strides[l * nl + x] != 0) == has(full.labels, sp.labels[x]));
        carries = carries || sp.strides[l * nl + x];
        base += digit[x] * sp.strides[l * nl + x];
      }
      CHECK(carries == (sp.sliced[l] != 0));
      if (!carries) {
        CHECK(red.labels == full.labels && red.dims == full.dims);
        continue;
      }
      // source strides of the remaining axes
      std::vector<u64> sstride;
      u64 stride = 1;
      for (size_t a = full.labels.size(); a-- > 0;) {
        if (!has(sp.labels, full.labels[a]))
          sstride.insert(sstride.begin(), stride);
        stride *= full.dims[a];
      }
      CHECK(sstride.size() == red.dims.size());
      for (u64 p = 0; p < red_elems; ++p) {
        // the kernel's decode of p (general form)
        u64 off = base, pstride = red_elems;
        std::vector<u64> coord(red.dims.size());
        for (size_t i = 0; i < red.dims.size(); ++i) {
          pstride /= red.dims[i];
          coord[i] = (p / pstride) % red.dims[i];
          off += coord[i] * sstride[i];
        }
        CHECK(off < full_elems);
        // the element meant: row-major index over the full leaf
        u64 want = 0;
        size_t r = 0;
        for (size_t a = 0; a < full.labels.size(); ++a) {
          u64 c;
          size_t x = std::find(sp.labels.begin(), sp.labels.end(),
                               full.labels[a]) - sp.labels.begin();
          if (x < nl)
            c = digit[x];
          else
            c = coord[r++];
          want = want * full.dims[a] + c;
        }
        CHECK(off == want);
      }
    }
  }
}

static void expect_refusal(const std::vector<LayoutTensor>& leaves,
                           const std::vector<u64>& pairs,
                           const std::vector<u64>& labels, const char* word) {
  SlicePlan sp;
  plan_slices(true, leaves, pairs.data(), pairs.size() / 2, labels.data(),
              labels.size(), &sp);
  CHECK(!sp.valid);
  CHECK(!sp.err.empty());
  if (!strstr(sp.err.c_str(), word)) {
    fprintf(stderr, "refusal '%s' lacks '%s'\n", sp.err.c_str(), word);
    exit(1);
  }
}

int main() {
  // A[i:3, s:3, k:5] B[k:5, t:2, j:7] C[s:3, t:2, l:5], slice (s, t)
  const u64 i = 1, s = 2, k = 3, t = 4, j = 5, l = 6;
  std::vector<LayoutTensor> abc = {tensor({i, s, k}, {3, 3, 5}),
                                   tensor({k, t, j}, {5, 2, 7}),
                                   tensor({s, t, l}, {3, 2, 5})};
  const std::vector<u64> path = {0, 1, 0, 2};
  {
    const std::vector<u64> labels = {s, t};
    SlicePlan sp;
    plan_slices(true, abc, path.data(), 2, labels.data(), 2, &sp);
    CHECK(sp.valid);
    CHECK(sp.count == 6);
    CHECK((sp.radices == std::vector<u64>{3, 2}));
    CHECK((sp.weights == std::vector<u64>{2, 1}));
    CHECK((sp.strides == std::vector<u64>{5, 0, 0, 7, 10, 5}));
    CHECK((sp.reduced[2].labels == std::vector<u64>{l}));
    CHECK(sp.layout.valid && sp.layout.out.size() == 2);
    CHECK((sp.layout.out[1].labels == std::vector<u64>{i, j, l}));
    check_gather(abc, sp);
  }
  {
    const std::vector<u64> labels = {t, s};
    SlicePlan sp;
    plan_slices(false, abc, path.data(), 2, labels.data(), 2, &sp);
    CHECK(sp.valid && sp.count == 6);
    CHECK((sp.weights == std::vector<u64>{3, 1}));
    check_gather(abc, sp);
  }
  {  // no labels: the plain plan, one assignment
    SlicePlan sp;
    plan_slices(true, abc, path.data(), 2, nullptr, 0, &sp);
    CHECK(sp.valid && sp.count == 1 && sp.strides.empty());
    CHECK(sp.reduced[0].labels == abc[0].labels);
    check_gather(abc, sp);
  }
  {  // a pow2 chain of rank-4 leaves, three labels on inner and outer axes
    std::vector<LayoutTensor> chain;
    std::vector<u64> pairs;
    const int n = 6;
    for (int x = 0; x < n; ++x)
      chain.push_back(tensor({100u + x, 200u + x, 300u + x, 101u + x},
                             {2, 4, 2, 2}));
    // close the chain's ends and pair up the 200/300 legs with partners
    for (int x = 0; x < n; ++x)
      chain.push_back(tensor({200u + x, 300u + x}, {4, 2}));
    chain.push_back(tensor({100u}, {2}));
    chain.push_back(tensor({100u + n}, {2}));
    for (size_t x = 1; x < chain.size(); ++x) {
      pairs.push_back(0);
      pairs.push_back(x);
    }
    const std::vector<u64> labels = {103, 201, 304};
    SlicePlan sp;
    plan_slices(true, chain, pairs.data(), pairs.size() / 2, labels.data(), 3,
                &sp);
    CHECK(sp.valid);
    CHECK(sp.count == 16);
    check_gather(chain, sp);
  }
  expect_refusal(abc, path, {99}, "no leaf");
  expect_refusal(abc, path, {s, s}, "twice");
  expect_refusal(abc, path, {j}, "final tensor");
  expect_refusal(abc, {0, 0, 0, 2}, {s}, "invalid contraction path");
  {
    std::vector<LayoutTensor> four = {
        tensor({1, 9}, {2, 2}), tensor({1, 9}, {2, 2}),
        tensor({2, 9}, {2, 2}), tensor({2, 9}, {2, 2})};
    expect_refusal(four, {0, 1, 2, 3, 0, 2}, {9}, "not two");
    std::vector<LayoutTensor> twice = {tensor({9, 9}, {2, 2})};
    expect_refusal(twice, {}, {9}, "repeated within leaf");
    const u64 big = 1ull << 33;
    std::vector<LayoutTensor> wide = {tensor({1, 2}, {big, big}),
                                      tensor({1, 2}, {big, big})};
    expect_refusal(wide, {0, 1}, {1, 2}, "overflows");
  }
  printf("slice_plan_check OK\n");
  return 0;
}
