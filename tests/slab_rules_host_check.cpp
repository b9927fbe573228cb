// The host rules the front ends of a grid in z-slabs share (vacancy_amd/csrc/slab_rules.h), as a program of its own, also
// under AddressSanitizer and UBSan (make slab_rules_host_check; driven by tests/test_slab_rules_host.py): the plan and the
// tie rule of the closing, which components stay, and the seam halo assembly of the distance field.  What must come out
// is written down as literals; the planes of the halo cases carry their own (z, i), so every plane that comes out is
// checked against the global slice it claims to be -- and every edge array is exactly as long as the rule says, so a read
// past one is the sanitizer's to report.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "slab_rules.h"

using namespace vcy::slab;

namespace {

int failures = 0, checks = 0;
const char* g_case = "";
#define EXPECT(what, want)                                                                                  \
  do {                                                                                                      \
    ++checks;                                                                                               \
    const long long got_ = (long long)(what), want_ = (long long)(want);                                    \
    if (got_ != want_) {                                                                                    \
      std::printf("FAILED %s:%d [%s]: %s = %lld, expected %lld\n", __FILE__, __LINE__, g_case, #what, got_, want_); \
      if (++failures > 40) std::exit(1);                                                                    \
    }                                                                                                       \
  } while (0)

// ---- the closing ---------------------------------------------------------------------------------------------------------
void closing() {
  g_case = "closing";
  double r = -1.0;
  int big_r = -1;
  long long sq = -1;
  EXPECT(close_hull_plan(1.3, 0.25f, &r, &big_r, &sq), kCloseOk);
  EXPECT(r == 1.3 * 0.25, 1);
  EXPECT(big_r, 4);
  EXPECT(close_hull_plan(2.0, 1.0f, &r, &big_r, &sq), kCloseOk);
  EXPECT(r == 2.0, 1);
  EXPECT(big_r, 4);
  EXPECT(close_hull_plan(125.0, 1.0f, &r, &big_r, &sq), kCloseOk);
  EXPECT(big_r, 127);
  const double ties[3] = {0.5, 1.5, 2.5};
  const long long squares[3] = {1, 4, 9};
  for (int i = 0; i < 3; ++i) {
    sq = -1;
    EXPECT(close_hull_plan(ties[i], 1.0f, &r, &big_r, &sq), kCloseTies);
    EXPECT(sq, squares[i]);
  }
  const double out_of_range[5] = {0.0, -1.0, 126.0, 125.5, std::nan("")};
  for (double rv : out_of_range) EXPECT(close_hull_plan(rv, 1.0f, &r, &big_r, &sq), kCloseOutOfRange);
  // (radius + 0.5)^2 = 7 is an integer, but no sum of three squares: no voxel lies at that distance
  const double seven = std::sqrt(7.0) - 0.5;
  EXPECT(std::fabs((seven + 0.5) * (seven + 0.5) - 7.0) <= 7e-9, 1);
  EXPECT(close_hull_plan(seven, 1.0f, &r, &big_r, &sq), kCloseOk);
  EXPECT(big_r, 5);
  // what the C++ facade passes: its float, widened
  EXPECT(close_hull_plan((double)1.5f, 1.0f, &r, &big_r, &sq), kCloseTies);
  EXPECT(close_hull_plan((double)1.3f, 1.0f, &r, &big_r, &sq), kCloseOk);
  EXPECT(r == (double)1.3f, 1);
  EXPECT(big_r, 4);
}

// ---- the keep rule -------------------------------------------------------------------------------------------------------
vcy_component comp(int64_t label, int64_t n_voxels) {
  vcy_component c = {};
  c.label = label, c.n_voxels = n_voxels;
  return c;
}

void expect_removed(const std::vector<vcy_component>& comps, int largest, int64_t min_voxels, std::vector<int> want,
                    long long want_n, long long want_voxels) {
  std::vector<uint8_t> removed(comps.size(), 7);
  int64_t n = -1, voxels = -1;
  select_components(comps.data(), (int64_t)comps.size(), largest, min_voxels, removed.data(), &n, &voxels);
  for (size_t i = 0; i < comps.size(); ++i) EXPECT(removed[i], want[i]);
  EXPECT(n, want_n);
  EXPECT(voxels, want_voxels);
}

void keep_rule() {
  g_case = "keep rule";
  const std::vector<vcy_component> comps = {comp(0, 4), comp(8, 2), comp(32, 2), comp(63, 1)};  // a tie: the lower label first
  expect_removed(comps, 0, 0, {0, 0, 0, 0}, 0, 0);
  expect_removed(comps, 1, 0, {0, 1, 1, 1}, 3, 5);
  expect_removed(comps, 2, 0, {0, 0, 1, 1}, 2, 3);
  expect_removed(comps, 9, 0, {0, 0, 0, 0}, 0, 0);   // more than there are
  expect_removed(comps, -3, 0, {0, 0, 0, 0}, 0, 0);  // negative: no rank limit, as 0
  expect_removed(comps, 0, 2, {0, 0, 0, 1}, 1, 1);   // exactly a component's size: it stays
  expect_removed(comps, 0, 3, {0, 1, 1, 1}, 3, 5);   // one above
  expect_removed(comps, 2, 3, {0, 1, 1, 1}, 3, 5);
  expect_removed(comps, 1, 5, {1, 1, 1, 1}, 4, 9);
  g_case = "keep rule, the empty list";
  int64_t n = -1, voxels = -1;
  select_components(nullptr, 0, 1, 0, nullptr, &n, &voxels);
  EXPECT(n, 0);
  EXPECT(voxels, 0);
  select_pieces(nullptr, 0, nullptr, nullptr, 0, nullptr);

  // three slabs: component 0 has a piece in every slab, 120 in the upper two, 50 is one piece of slab 0
  g_case = "keep rule, pieces";
  const std::vector<vcy_component> merged = {comp(0, 30), comp(120, 12), comp(50, 5)};
  const std::vector<int64_t> global = {0, 50, /* slab 1 */ 0, 120, /* slab 2 */ 0, 120};
  struct { int largest; int64_t min_voxels; int want[6]; } cases[4] = {
      {1, 0, {0, 1, 0, 1, 0, 1}}, {0, 10, {0, 1, 0, 0, 0, 0}}, {2, 13, {0, 1, 0, 1, 0, 1}}, {1, 31, {1, 1, 1, 1, 1, 1}}};
  for (const auto& c : cases) {
    std::vector<uint8_t> removed(3, 7), pieces(6, 7);
    select_components(merged.data(), 3, c.largest, c.min_voxels, removed.data(), &n, &voxels);
    select_pieces(merged.data(), 3, removed.data(), global.data(), 6, pieces.data());
    for (int k = 0; k < 6; ++k) EXPECT(pieces[k], c.want[k]);
  }
}

// ---- the seam halo assembly ----------------------------------------------------------------------------------------------
constexpr int kPlane = 3;
uint16_t value_of(int z, int i) { return (uint16_t)(z * 8 + i + 1); }

struct Grid {
  std::vector<int32_t> bounds;
  int radius;
  std::vector<std::vector<uint16_t>> bottoms, tops;  // min(radius, own slices) planes each, no more
  std::vector<const uint16_t*> bottom_of, top_of;
  Grid(std::vector<int32_t> b, int r) : bounds(b), radius(r) {
    const int ns = (int)bounds.size() - 1;
    bottoms.resize(ns), tops.resize(ns);
    for (int s = 0; s < ns; ++s) {
      const int m = std::min(radius, bounds[s + 1] - bounds[s]);
      for (int k = 0; k < m; ++k)
        for (int i = 0; i < kPlane; ++i) {
          bottoms[s].push_back(value_of(bounds[s] + k, i));
          tops[s].push_back(value_of(bounds[s + 1] - m + k, i));
        }
      bottom_of.push_back(s > 0 ? bottoms[s].data() : nullptr);  // nobody needs the grid's own two ends
      top_of.push_back(s + 1 < ns ? tops[s].data() : nullptr);
    }
  }
  int n_slabs() const { return (int)bounds.size() - 1; }
  // the halo of `slab`, every plane checked against its global slice; returns the status
  Halo halo(int slab, int want_below, int want_above) const {
    const int nz = bounds.back();
    std::vector<uint16_t> below((size_t)kPlane * want_below, 0), above((size_t)kPlane * want_above, 0);
    int nb = -1, na = -1;
    const Halo rc = distance_halo(n_slabs(), bounds.data(), radius, kPlane, bottom_of.data(), top_of.data(), slab,
                                  want_below ? below.data() : nullptr, want_above ? above.data() : nullptr, &nb, &na);
    if (rc != kHaloOk) return rc;
    EXPECT(nb, want_below);
    EXPECT(na, want_above);
    EXPECT(nb, std::min(radius, bounds[slab]));
    EXPECT(na, std::min(radius, nz - bounds[slab + 1]));
    for (int k = 0; k < nb; ++k)
      for (int i = 0; i < kPlane; ++i) EXPECT(below[(size_t)k * kPlane + i], value_of(bounds[slab] - nb + k, i));
    for (int k = 0; k < na; ++k)
      for (int i = 0; i < kPlane; ++i) EXPECT(above[(size_t)k * kPlane + i], value_of(bounds[slab + 1] + k, i));
    return rc;
  }
};

void halos() {
  g_case = "halo: 17 slices, [0, 6, 8, 10, 17], R = 12";
  {
    const Grid g({0, 6, 8, 10, 17}, 12);
    const int below[4] = {0, 6, 8, 10}, above[4] = {11, 9, 7, 0};  // [8, 10): 8 from [6, 8) and [0, 6), 7 from [10, 17)
    for (int s = 0; s < 4; ++s) EXPECT(g.halo(s, below[s], above[s]), kHaloOk);
  }
  g_case = "halo: 23 slices in steps of 2, R = 127";
  {
    std::vector<int32_t> b;
    for (int z = 0; z < 23; z += 2) b.push_back(z);
    b.push_back(23);
    const Grid g(b, 127);
    EXPECT(g.n_slabs(), 12);
    for (int s = 0; s < g.n_slabs(); ++s) EXPECT(g.halo(s, b[s], 23 - b[s + 1]), kHaloOk);  // the whole rest of the grid
  }
  g_case = "halo: a single slab";
  {
    const Grid g({0, 9}, 5);
    EXPECT(g.halo(0, 0, 0), kHaloOk);
    int nb = -1, na = -1;
    EXPECT(distance_halo(1, g.bounds.data(), 5, kPlane, nullptr, nullptr, 0, nullptr, nullptr, &nb, &na), kHaloOk);
    EXPECT(nb, 0);
    EXPECT(na, 0);
  }
  g_case = "halo: R = 1";
  {
    const Grid g({0, 6, 8, 10, 17}, 1);
    for (int s = 0; s < 4; ++s) EXPECT(g.halo(s, s > 0, s < 3), kHaloOk);
  }
  g_case = "halo: refusals";
  {
    Grid g({0, 6, 8, 10, 17}, 12);
    EXPECT(g.halo(-1, 0, 0), kHaloBadSlab);
    EXPECT(g.halo(4, 0, 0), kHaloBadSlab);
    g.top_of[0] = nullptr;  // slab [8, 10) reaches down into [0, 6); slab [6, 8) needs it too, slab 0 itself does not
    EXPECT(g.halo(2, 8, 7), kHaloMissingEdge);
    EXPECT(g.halo(1, 6, 9), kHaloMissingEdge);
    EXPECT(g.halo(0, 0, 11), kHaloOk);
    g.top_of[0] = g.tops[0].data();
    g.bottom_of[3] = nullptr;
    EXPECT(g.halo(2, 8, 7), kHaloMissingEdge);
    EXPECT(g.halo(3, 10, 0), kHaloOk);
    g.bottom_of[3] = g.bottoms[3].data();
    EXPECT(g.halo(2, 8, 7), kHaloOk);
    int nb = -1, na = -1;
    std::vector<uint16_t> buf((size_t)kPlane * 12);
    EXPECT(distance_halo(4, g.bounds.data(), 12, kPlane, g.bottom_of.data(), g.top_of.data(), 2, nullptr, buf.data(), &nb, &na),
           kHaloBadArgument);  // 8 planes to come and nowhere to put them
    EXPECT(distance_halo(4, g.bounds.data(), 0, kPlane, g.bottom_of.data(), g.top_of.data(), 2, buf.data(), buf.data(), &nb, &na),
           kHaloBadArgument);
    EXPECT(distance_halo(0, g.bounds.data(), 12, kPlane, g.bottom_of.data(), g.top_of.data(), 0, buf.data(), buf.data(), &nb, &na),
           kHaloBadArgument);
    const Grid from_one({1, 6, 8}, 3), level({0, 6, 6, 8}, 3), falling({0, 6, 5, 8}, 3);
    EXPECT(from_one.halo(0, 0, 0), kHaloBadBounds);
    EXPECT(level.halo(0, 0, 0), kHaloBadBounds);
    EXPECT(falling.halo(2, 0, 0), kHaloBadBounds);
  }
}

}  // namespace

int main() {
  closing();
  keep_rule();
  halos();
  std::printf("slab_rules_host_check: %d checks, %d failures\n", checks, failures);
  return failures ? 1 : 0;
}
