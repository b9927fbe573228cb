// Stand-alone check of vcy_decimate_mesh_quadric_host (vacancy_amd/csrc/mesh_decimate_host.hip, mesh_quadric.h) and the
// vcy_mesh_normals_host behind it (mesh_host.hip) for a host sanitizer build: no GPU, no HIP runtime, its own
// vcy::set_error.  `make -C vacancy_amd/csrc quadric_host_check` builds the three files with AddressSanitizer and UBSan on the
// host side and runs the program (CPU only).  The meshes are generated here: the tessellated box of tests/quadric_cases.py
// (12 x 12 quads per side), the shallow wedge, member rows of 1, 16, 17, 48, 49, 256 and 257 vertices, zero-area faces;
// output arrays are exactly as long as the contract says.  Faces and maps are compared with vcy_decimate_mesh_host's MEAN;
// the box has to stay on its surface; the wedge has to fall back everywhere; then the refusals.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

#include "vacancy_hip.h"

namespace vcy {
thread_local char g_error[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}
}  // namespace vcy

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      return 1;                                                      \
    }                                                                \
  } while (0)

namespace {

struct TestMesh {
  std::vector<float> v;
  std::vector<int32_t> f;
  int64_t nv() const { return (int64_t)v.size() / 3; }
  int64_t nf() const { return (int64_t)f.size() / 3; }
};

struct Result {
  std::vector<float> v, vn, fn;
  std::vector<int32_t> f, vmap, src;
  int64_t nv = -1, nf = -1, fallbacks = -1;
};

vcy_decimate_option option(float cell, float origin, int mode = VCY_DECIMATE_MEAN) {
  vcy_decimate_option o;
  o.cell = cell;
  o.origin[0] = o.origin[1] = o.origin[2] = origin;
  o.mode = mode;
  return o;
}

void prepare(const TestMesh& m, Result* r) {
  r->v.assign(m.v.size(), 77.0f);
  r->f.assign(m.f.size(), 77);
  r->vmap.assign((size_t)m.nv(), 77);
  r->src.assign((size_t)m.nf(), 77);
  r->vn.assign(m.v.size(), 77.0f);
  r->fn.assign(m.f.size(), 77.0f);
  r->nv = r->nf = r->fallbacks = -1;
}

int quadric(const TestMesh& m, const vcy_decimate_option& o, float reg, Result* r, bool optional = true) {
  prepare(m, r);
  return vcy_decimate_mesh_quadric_host(m.nv(), m.nf(), m.v.data(), m.f.data(), &o, reg, r->v.data(), r->f.data(), &r->nv, &r->nf,
                                        optional ? r->vmap.data() : nullptr, optional ? r->src.data() : nullptr,
                                        optional ? r->vn.data() : nullptr, optional ? r->fn.data() : nullptr,
                                        optional ? &r->fallbacks : nullptr);
}

int mean(const TestMesh& m, const vcy_decimate_option& o, Result* r) {
  prepare(m, r);
  return vcy_decimate_mesh_host(m.nv(), m.nf(), m.v.data(), m.f.data(), &o, r->v.data(), r->f.data(), &r->nv, &r->nf, r->vmap.data(),
                                r->src.data(), r->vn.data(), r->fn.data());
}

bool untouched(const Result& r) {
  for (float x : r.v) if (x != 77.0f) return false;
  for (float x : r.vn) if (x != 77.0f) return false;
  for (float x : r.fn) if (x != 77.0f) return false;
  for (int32_t x : r.f) if (x != 77) return false;
  for (int32_t x : r.vmap) if (x != 77) return false;
  for (int32_t x : r.src) if (x != 77) return false;
  return r.nv == -1 && r.nf == -1 && r.fallbacks == -1;
}

// faces, maps and counts of the MEAN call; nothing behind the counts; the positions of `n_same` or more vertices its bits
bool same_but_positions(const Result& q, const Result& m, int64_t* n_same) {
  if (q.nv != m.nv || q.nf != m.nf || q.f != m.f || q.vmap != m.vmap || q.src != m.src) return false;
  for (size_t i = (size_t)(3 * q.nv); i < q.v.size(); ++i) if (q.v[i] != 77.0f) return false;
  *n_same = 0;
  for (int64_t i = 0; i < q.nv; ++i) *n_same += std::memcmp(&q.v[3 * (size_t)i], &m.v[3 * (size_t)i], 3 * sizeof(float)) == 0;
  return true;
}

const double kLo = -3.1, kHi = 4.3;

TestMesh box() {
  TestMesh m;
  const int n = 12;
  std::map<std::tuple<int, int, int>, int> ids;
  const auto vid = [&](int axis, int a, int b, int side, int ii, int jj) {
    int ijk[3];
    ijk[axis] = side * n, ijk[a] = ii, ijk[b] = jj;
    const auto key = std::make_tuple(ijk[0], ijk[1], ijk[2]);
    const auto it = ids.find(key);
    if (it != ids.end()) return it->second;
    const int id = (int)ids.size();
    ids[key] = id;
    for (int c = 0; c < 3; ++c) m.v.push_back((float)(kLo + (kHi - kLo) * ijk[c] / n));
    return id;
  };
  for (int axis = 0; axis < 3; ++axis) {
    const int a = axis == 0 ? 1 : 0, b = axis == 2 ? 1 : 2;
    for (int side = 0; side < 2; ++side)
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
          int q[4] = {vid(axis, a, b, side, i, j), vid(axis, a, b, side, i + 1, j), vid(axis, a, b, side, i + 1, j + 1),
                      vid(axis, a, b, side, i, j + 1)};
          if ((side == 1) == (axis != 1)) std::swap(q[0], q[3]), std::swap(q[1], q[2]);
          m.f.insert(m.f.end(), {q[0], q[1], q[2], q[0], q[2], q[3]});
        }
  }
  return m;
}

double box_distance(const float* p) {
  double out2 = 0.0, in = 1e30;
  for (int c = 0; c < 3; ++c) {
    const double x = (double)p[c], lo = (double)(float)kLo, hi = (double)(float)kHi;
    const double q = std::min(std::max(x, lo), hi);
    out2 += (x - q) * (x - q);
    in = std::min(in, std::min(x - lo, hi - x));
  }
  return out2 > 0.0 ? std::sqrt(out2) : std::fabs(in);
}

double worst_distance(const Result& r) {
  double worst = 0.0;
  for (int64_t i = 0; i < r.nv; ++i) worst = std::max(worst, box_distance(&r.v[3 * (size_t)i]));
  return worst;
}

void add_sheet(TestMesh* m, double slope) {
  const int base = (int)m->nv();
  for (int i = 0; i < 9; ++i)
    for (int j = 0; j < 9; ++j) {
      const float x = (float)i * 0.4f - 1.0f, y = (float)j * 0.4f - 1.0f;
      m->v.insert(m->v.end(), {x, y, (float)(slope * ((double)x - 40.0))});
    }
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 8; ++j) {
      const int a = base + i * 9 + j;
      m->f.insert(m->f.end(), {a, a + 9, a + 10, a, a + 10, a + 1});
    }
}

}  // namespace

int main() {
  Result q, m;
  int64_t same = 0;

  // the box: faces and maps of MEAN, no fallback at 1e-3, on the surface where the mean is a quarter of a cell inside
  const TestMesh bx = box();
  CHECK(bx.nv() == 866 && bx.nf() == 1728);
  const float cells[2] = {2.0f, 3.7f};
  const int64_t want_nv[2] = {56, 26};
  for (int ci = 0; ci < 2; ++ci) {
    const vcy_decimate_option o = option(cells[ci], -13.25f);
    CHECK(mean(bx, o, &m) == VCY_OK && m.nv == want_nv[ci]);
    CHECK(quadric(bx, o, 1e-3f, &q) == VCY_OK && same_but_positions(q, m, &same));
    CHECK(q.fallbacks == 0);
    CHECK(worst_distance(q) <= worst_distance(m) / 20.0);
    for (int64_t i = 0; i < 3 * q.nv; ++i) CHECK(q.vn[(size_t)i] != 77.0f);
    CHECK(quadric(bx, o, 0.0f, &q) == VCY_OK && same_but_positions(q, m, &same));   // flats and edges fall back, corners do not
    CHECK(q.fallbacks == q.nv - 8 && same >= q.fallbacks);
    CHECK(quadric(bx, o, 1.0f, &q) == VCY_OK && same_but_positions(q, m, &same) && q.fallbacks == 0);
    CHECK(quadric(bx, o, 1e-3f, &q, false) == VCY_OK && q.nv == m.nv && q.fallbacks == -1 && q.vmap[0] == 77 && q.vn[0] == 77.0f);
  }

  // the wedge: the planes meet far outside every cell, every output vertex keeps the mean's bits
  TestMesh wedge;
  add_sheet(&wedge, 0.02);
  add_sheet(&wedge, -0.02);
  for (float reg : {0.0f, 1e-3f}) {
    const vcy_decimate_option o = option(3.7f, -13.25f);
    CHECK(mean(wedge, o, &m) == VCY_OK && m.nv == 4);
    CHECK(quadric(wedge, o, reg, &q) == VCY_OK && same_but_positions(q, m, &same));
    CHECK(q.fallbacks == 4 && same == 4);
  }

  // member rows of 1 .. 257 vertices, one cell each along z, every vertex in a face with two vertices of a ring; behind them
  // zero-area faces and a face that names a vertex twice
  TestMesh tiers;
  const int sizes[7] = {1, 16, 17, 48, 49, 256, 257};
  int total = 0;
  for (int k = 0; k < 7; ++k)
    for (int i = 0; i < sizes[k]; ++i, ++total)
      tiers.v.insert(tiers.v.end(), {1.8f + 0.5f * (float)((total * 37) % 643) / 643.0f, 1.8f + 0.5f * (float)((total * 101) % 643) / 643.0f,
                                     -12.2f + 2.0f * (float)k + 0.5f * (float)((total * 211) % 643) / 643.0f});
  CHECK(total == 644);
  for (int k = 0; k < 16; ++k) {
    const float a = 6.2831853f * (float)k / 16.0f;
    tiers.v.insert(tiers.v.end(), {2.05f + 6.0f * std::cos(a), 2.05f + 6.0f * std::sin(a), 2.05f});
  }
  for (int k = 0; k < total; ++k) {
    const int i = (k * 13) % total;
    tiers.f.insert(tiers.f.end(), {i, total + i % 16, total + (i + 1) % 16});
  }
  tiers.v.insert(tiers.v.end(), {-4.0f, -5.0f, 5.0f, -1.0f, -5.0f, 5.0f, 2.0f, -5.0f, 5.0f});
  tiers.f.insert(tiers.f.end(), {660, 661, 662, 660, 660, 662, 3, 3, 4});
  for (float reg : {0.0f, 1e-3f, 1.0f}) {
    const vcy_decimate_option o = option(2.0f, -13.25f);
    CHECK(mean(tiers, o, &m) == VCY_OK && m.nv == 7 + 16 + 3);
    CHECK(quadric(tiers, o, reg, &q) == VCY_OK && same_but_positions(q, m, &same));
    CHECK(q.fallbacks >= 3 && q.fallbacks <= q.nv && same >= q.fallbacks);          // the three on the line have no area around them
    for (int i = 660; i < 663; ++i)
      CHECK(std::memcmp(&q.v[3 * (size_t)q.vmap[(size_t)i]], &m.v[3 * (size_t)m.vmap[(size_t)i]], 3 * sizeof(float)) == 0);
    if (reg > 0.0f) CHECK(same < q.nv);
  }

  // nothing to do
  {
    int64_t a = -1, b = -1, c = -1;
    const vcy_decimate_option o = option(2.0f, 0.0f);
    CHECK(vcy_decimate_mesh_quadric_host(0, 0, nullptr, nullptr, &o, 1e-3f, nullptr, nullptr, &a, &b, nullptr, nullptr, nullptr, nullptr, &c) == VCY_OK);
    CHECK(a == 0 && b == 0 && c == 0);
  }

  // refusals: nothing is written, not the counts, not the fallback count
  TestMesh oct;
  oct.v = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
  oct.f = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
  const auto refused = [&](const TestMesh& mesh, const vcy_decimate_option& o, float reg) {
    return quadric(mesh, o, reg, &q) == VCY_ERR_INVALID_ARG && untouched(q);
  };
  CHECK(quadric(oct, option(1.0f, 0.0f), 1e-3f, &q) == VCY_OK && q.nv == 6 && q.nf == 8);
  CHECK(refused(oct, option(1.0f, 0.0f, VCY_DECIMATE_NEAREST), 1e-3f));
  CHECK(std::strstr(vcy::g_error, "mode") != nullptr);
  CHECK(refused(oct, option(1.0f, 0.0f, VCY_DECIMATE_FIRST), 1e-3f));
  CHECK(refused(oct, option(1.0f, 0.0f, 3), 1e-3f));
  CHECK(refused(oct, option(1.0f, 0.0f, -1), 1e-3f));
  CHECK(refused(oct, option(1.0f, 0.0f), std::nanf("")));
  CHECK(std::strstr(vcy::g_error, "regularize") != nullptr);
  CHECK(refused(oct, option(1.0f, 0.0f), INFINITY));
  CHECK(refused(oct, option(1.0f, 0.0f), -1e-6f));
  CHECK(refused(oct, option(1.0f, 0.0f), std::nextafter(1.0f, 2.0f)));
  CHECK(refused(oct, option(0.0f, 0.0f), 1e-3f));
  CHECK(std::strstr(vcy::g_error, "cell") != nullptr);
  CHECK(refused(oct, option(1.0f, std::nanf("")), 1e-3f));
  TestMesh bad = oct;
  bad.f[7] = 6;
  CHECK(refused(bad, option(1.0f, 0.0f), 1e-3f));
  CHECK(std::strstr(vcy::g_error, "face 2") != nullptr);
  bad.f[7] = -1;
  CHECK(refused(bad, option(1.0f, 0.0f), 1e-3f));
  bad = oct;
  bad.v[4] = std::nanf("");
  CHECK(refused(bad, option(1.0f, 0.0f), 1e-3f));
  CHECK(std::strstr(vcy::g_error, "vertex 1") != nullptr);
  bad.v[4] = INFINITY;
  CHECK(refused(bad, option(1.0f, 0.0f), 1e-3f));
  bad.v[4] = 1073741760.0f;  // the float below 2^30 cells: fine, and the quadric of a face that long stays finite
  CHECK(quadric(bad, option(1.0f, 0.0f), 1e-3f, &q) == VCY_OK && q.nv == 6);
  bad.v[4] = 3.0e38f;        // squares of areas beyond the doubles' float range, not beyond the doubles
  bad.v[0] = -3.0e38f;
  CHECK(quadric(bad, option(1.0e30f, 0.0f), 1e-3f, &q) == VCY_OK);
  {
    const vcy_decimate_option o = option(1.0f, 0.0f);
    int64_t a = -1, b = -1, c = -1;
    std::vector<float> vo(oct.v.size(), 77.0f);
    std::vector<int32_t> fo(oct.f.size(), 77);
    CHECK(vcy_decimate_mesh_quadric_host(oct.nv(), (int64_t)1 << 30, oct.v.data(), oct.f.data(), &o, 1e-3f, vo.data(), fo.data(), &a, &b, nullptr, nullptr, nullptr, nullptr, &c) == VCY_ERR_UNSUPPORTED);
    CHECK(vcy_decimate_mesh_quadric_host(oct.nv(), oct.nf(), oct.v.data(), oct.f.data(), nullptr, 1e-3f, vo.data(), fo.data(), &a, &b, nullptr, nullptr, nullptr, nullptr, &c) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_decimate_mesh_quadric_host(oct.nv(), oct.nf(), oct.v.data(), oct.f.data(), &o, 1e-3f, nullptr, fo.data(), &a, &b, nullptr, nullptr, nullptr, nullptr, &c) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_decimate_mesh_quadric_host(oct.nv(), oct.nf(), oct.v.data(), oct.f.data(), &o, 1e-3f, vo.data(), fo.data(), nullptr, &b, nullptr, nullptr, nullptr, nullptr, &c) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_decimate_mesh_quadric_host(-1, oct.nf(), oct.v.data(), oct.f.data(), &o, 1e-3f, vo.data(), fo.data(), &a, &b, nullptr, nullptr, nullptr, nullptr, &c) == VCY_ERR_INVALID_ARG);
    CHECK(a == -1 && b == -1 && c == -1 && vo[0] == 77.0f && fo[0] == 77);
  }

  std::puts("quadric_host_check: ok");
  return 0;
}
