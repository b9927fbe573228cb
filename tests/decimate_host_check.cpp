// Stand-alone check of vcy_decimate_mesh_host (vacancy_amd/csrc/mesh_decimate_host.hip) and the vcy_mesh_normals_host behind
// it (mesh_host.hip) for a host sanitizer build: no GPU, no HIP runtime, its own vcy::set_error.  `make -C vacancy_amd/csrc
// decimate_host_check` builds the three files with AddressSanitizer and UBSan on the host side and runs the program (CPU
// only).  The meshes are generated here -- the cases of tests/decimate_cases.py that need no random numbers and no
// oracle: an octahedron, the open patch, two sheets with equal and with opposite orientation, rotations of one face, the
// patch on cell planes with -0.0, a crowd of 700 vertices in one cell, degenerate faces, vertices no face names -- and run
// over the cells 0.001, 0.75, 2.0, 3.7, 1000 and the three modes; output arrays are exactly as long as the contract says.
// The counts are those of the numpy restatement (tests/decimate_ref.py); every output is checked for the properties of
// the definition.
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <set>
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

const float kCells[5] = {0.001f, 0.75f, 2.0f, 3.7f, 1000.0f};

struct TestMesh {
  std::vector<float> v;
  std::vector<int32_t> f;
  int64_t nv() const { return (int64_t)v.size() / 3; }
  int64_t nf() const { return (int64_t)f.size() / 3; }
};

struct Result {
  std::vector<float> v, vn, fn;
  std::vector<int32_t> f, vmap, src;
  int64_t nv = -1, nf = -1;
};

vcy_decimate_option option(float cell, float origin, int mode) {
  vcy_decimate_option o;
  o.cell = cell;
  o.origin[0] = o.origin[1] = o.origin[2] = origin;
  o.mode = mode;
  return o;
}

int decimate(const TestMesh& m, const vcy_decimate_option& o, Result* r, bool maps = true, bool normals = true) {
  r->v.assign(m.v.size(), 77.0f);
  r->f.assign(m.f.size(), 77);
  r->vmap.assign((size_t)m.nv(), 77);
  r->src.assign((size_t)m.nf(), 77);
  r->vn.assign(m.v.size(), 77.0f);
  r->fn.assign(m.f.size(), 77.0f);
  r->nv = r->nf = -1;
  return vcy_decimate_mesh_host(m.nv(), m.nf(), m.v.data(), m.f.data(), &o, r->v.data(), r->f.data(), &r->nv, &r->nf,
                                maps ? r->vmap.data() : nullptr, maps ? r->src.data() : nullptr,
                                normals ? r->vn.data() : nullptr, normals ? r->fn.data() : nullptr);
}

bool untouched(const Result& r) {
  for (float x : r.v) if (x != 77.0f) return false;
  for (float x : r.vn) if (x != 77.0f) return false;
  for (float x : r.fn) if (x != 77.0f) return false;
  for (int32_t x : r.f) if (x != 77) return false;
  for (int32_t x : r.vmap) if (x != 77) return false;
  for (int32_t x : r.src) if (x != 77) return false;
  return r.nv == -1 && r.nf == -1;
}

// the properties of the definition that need no second implementation
bool well_formed(const TestMesh& m, const Result& r) {
  if (r.nv < 0 || r.nf < 0 || r.nv > m.nv() || r.nf > m.nf()) return false;
  std::set<std::tuple<int, int, int>> seen;
  std::vector<char> named((size_t)r.nv, 0);
  for (int64_t g = 0; g < r.nf; ++g) {
    const int32_t* t = &r.f[3 * (size_t)g];
    if (t[0] < 0 || t[1] < 0 || t[2] < 0 || t[0] >= r.nv || t[1] >= r.nv || t[2] >= r.nv) return false;
    if (t[0] == t[1] || t[1] == t[2] || t[2] == t[0]) return false;
    const int s = (t[0] < t[1] && t[0] < t[2]) ? 0 : (t[1] < t[2] ? 1 : 2);
    if (!seen.insert(std::make_tuple(t[s], t[(s + 1) % 3], t[(s + 2) % 3])).second) return false;
    named[(size_t)t[0]] = named[(size_t)t[1]] = named[(size_t)t[2]] = 1;
    const int32_t src = r.src[(size_t)g];
    if (src < 0 || src >= m.nf() || (g > 0 && src <= r.src[(size_t)g - 1])) return false;
    for (int j = 0; j < 3; ++j)
      if (r.vmap[(size_t)m.f[3 * (size_t)src + j]] != t[j]) return false;
  }
  for (char c : named) if (!c) return false;
  for (int32_t x : r.vmap) if (x < -1 || x >= r.nv) return false;
  for (size_t i = (size_t)(3 * r.nv); i < r.v.size(); ++i) if (r.v[i] != 77.0f) return false;   // nothing behind the counts
  for (size_t i = (size_t)(3 * r.nf); i < r.f.size(); ++i) if (r.f[i] != 77) return false;
  return true;
}

TestMesh patch(const float* ax, bool plane_z) {
  TestMesh m;
  for (int y = 0; y < 9; ++y)
    for (int x = 0; x < 9; ++x) {
      const float z = plane_z ? ((x + y) % 2 == 0 ? -0.0f : -1.5f) : (float)(0.05 * (x * x + 0.5 * y * y));
      m.v.insert(m.v.end(), {ax ? ax[x] : (float)x, ax ? ax[y] : (float)y, z});
    }
  for (int y = 0; y < 8; ++y)
    for (int x = 0; x < 8; ++x) {
      const int a = 9 * y + x, b = a + 1, c = a + 9, d = a + 10;
      m.f.insert(m.f.end(), {a, b, d, a, d, c});
    }
  return m;
}

TestMesh two_sheets(bool opposite) {
  TestMesh m = patch(nullptr, false);
  const size_t nv = m.v.size() / 3, nf = m.f.size() / 3;
  for (size_t i = 0; i < nv; ++i) m.v.insert(m.v.end(), {m.v[3 * i], m.v[3 * i + 1], m.v[3 * i + 2] + 0.01f});
  for (size_t i = 0; i < nf; ++i) {
    const int a = m.f[3 * i] + (int)nv, b = m.f[3 * i + 1] + (int)nv, c = m.f[3 * i + 2] + (int)nv;
    if (opposite) m.f.insert(m.f.end(), {c, b, a});
    else m.f.insert(m.f.end(), {a, b, c});
  }
  return m;
}

struct Expected {
  int64_t nv[5], nf[5];  // per cell of kCells
};

int run_matrix(const char* name, const TestMesh& m, float origin, const Expected& want) {
  Result r, first;
  for (int ci = 0; ci < 5; ++ci)
    for (int mode = 0; mode < 3; ++mode) {
      const vcy_decimate_option o = option(kCells[ci], origin, mode);
      if (decimate(m, o, &r) != VCY_OK || !well_formed(m, r) || r.nv != want.nv[ci] || r.nf != want.nf[ci]) {
        std::fprintf(stderr, "%s cell %g mode %d: %lld vertices, %lld faces, expected %lld, %lld (%s)\n", name, (double)kCells[ci], mode,
                     (long long)r.nv, (long long)r.nf, (long long)want.nv[ci], (long long)want.nf[ci], vcy::g_error);
        return 1;
      }
      for (int64_t i = 0; i < 3 * r.nf; ++i) CHECK(r.fn[(size_t)i] != 77.0f);
      for (int64_t i = 0; i < 3 * r.nv; ++i) CHECK(r.vn[(size_t)i] != 77.0f);
      // faces and maps do not depend on the mode
      if (mode == 0) first = r;
      else CHECK(first.f == r.f && first.vmap == r.vmap && first.src == r.src);
    }
  return 0;
}

}  // namespace

int main() {
  Result r;

  TestMesh oct;
  oct.v = {1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1, 0, 0, 0, 1, 0, 0, -1};
  oct.f = {0, 2, 4, 2, 1, 4, 1, 3, 4, 3, 0, 4, 2, 0, 5, 1, 2, 5, 3, 1, 5, 0, 3, 5};
  // cells of edge 2 from -13.25 have a plane at 0.75: the three vertices at -1 share the cell of the origin
  CHECK(run_matrix("octahedron", oct, -13.25f, Expected{{6, 6, 4, 0, 0}, {8, 8, 4, 0, 0}}) == 0);
  {  // a fine lattice returns the mesh: bits, faces, identity maps
    CHECK(decimate(oct, option(0.001f, -13.25f, VCY_DECIMATE_NEAREST), &r) == VCY_OK && r.nv == 6 && r.nf == 8);
    CHECK(std::memcmp(r.v.data(), oct.v.data(), oct.v.size() * sizeof(float)) == 0 && r.f == oct.f);
    for (int i = 0; i < 6; ++i) CHECK(r.vmap[(size_t)i] == i);
    for (int i = 0; i < 8; ++i) CHECK(r.src[(size_t)i] == i);
    for (size_t i = 0; i < r.vn.size(); ++i) CHECK(std::fabs(r.vn[i] - oct.v[i]) < 1e-6f);
  }

  const TestMesh open_patch = patch(nullptr, false);
  CHECK(run_matrix("open_patch", open_patch, -13.25f, Expected{{81, 81, 34, 12, 0}, {128, 128, 47, 13, 0}}) == 0);
  CHECK(run_matrix("two_sheets_same", two_sheets(false), -13.25f, Expected{{162, 81, 34, 12, 0}, {256, 128, 47, 13, 0}}) == 0);
  CHECK(run_matrix("two_sheets_opposite", two_sheets(true), -13.25f, Expected{{162, 81, 34, 12, 0}, {256, 256, 94, 26, 0}}) == 0);

  TestMesh rot;
  rot.v = {-9.0f, -9.0f, -9.0f, 9.5f, -8.0f, -7.0f, 0.5f, 9.0f, -8.5f, 1.0f, 0.5f, 10.0f};
  rot.f = {0, 1, 2, 1, 2, 0, 2, 0, 1, 0, 2, 1, 0, 1, 3};
  CHECK(run_matrix("rotations", rot, -13.25f, Expected{{4, 4, 4, 4, 0}, {3, 3, 3, 3, 0}}) == 0);
  CHECK(decimate(rot, option(2.0f, -13.25f, VCY_DECIMATE_FIRST), &r) == VCY_OK);
  CHECK(r.src[0] == 0 && r.src[1] == 3 && r.src[2] == 4);  // the two other rotations go, the mirror image stays

  const float axis[9] = {-7.4f, -6.0f, -3.0f, -1.5f, -0.0f, 1.5f, 3.0f, 6.0f, 7.4f};
  const TestMesh boundary = patch(axis, true);
  CHECK(run_matrix("boundary", boundary, 0.0f, Expected{{81, 81, 73, 46, 8}, {128, 128, 120, 96, 18}}) == 0);
  CHECK(decimate(boundary, option(0.001f, 0.0f, VCY_DECIMATE_FIRST), &r) == VCY_OK);
  CHECK(std::memcmp(r.v.data(), boundary.v.data(), boundary.v.size() * sizeof(float)) == 0);  // -0.0 keeps its sign
  CHECK(decimate(boundary, option(0.001f, 0.0f, VCY_DECIMATE_MEAN), &r) == VCY_OK);
  CHECK(r.v[2] == 0.0f && !std::signbit(r.v[2]) && std::signbit(boundary.v[2]));               // +0 + -0.0

  // 700 vertices in one cell, each in a face with two vertices of a ring in other cells; then vertices no face names
  // and degenerate faces behind them
  TestMesh crowd;
  for (int i = 0; i < 700; ++i)
    crowd.v.insert(crowd.v.end(), {1.8f + 0.5f * (float)((i * 37) % 700) / 700.0f, 1.8f + 0.5f * (float)((i * 101) % 700) / 700.0f,
                                   1.8f + 0.5f * (float)((i * 211) % 700) / 700.0f});
  for (int k = 0; k < 16; ++k) {
    const float a = 6.2831853f * (float)k / 16.0f;
    crowd.v.insert(crowd.v.end(), {2.05f + 6.0f * std::cos(a), 2.05f + 6.0f * std::sin(a), 2.05f});
  }
  for (int k = 0; k < 700; ++k) {
    const int i = (k * 13) % 700;
    crowd.f.insert(crowd.f.end(), {i, 700 + i % 16, 700 + (i + 1) % 16});
  }
  crowd.v.insert(crowd.v.end(), {-9.0f, 0.5f, 2.0f, 40.0f, 40.0f, 40.0f});
  crowd.f.insert(crowd.f.end(), {3, 3, 4, 5, 5, 5, 700, 701, 700});
  for (int mode = 0; mode < 3; ++mode) {
    CHECK(decimate(crowd, option(2.0f, -13.25f, mode), &r) == VCY_OK && well_formed(crowd, r));
    CHECK(r.nv == 17 && r.nf == 16);                      // the crowd is one vertex, 684 faces are duplicates, 3 collapse
    CHECK(r.vmap[716] == -1 && r.vmap[717] == -1);
    for (int i = 0; i < 700; ++i) CHECK(r.vmap[(size_t)i] == r.vmap[0]);
    const float* p = &r.v[3 * (size_t)r.vmap[0]];
    for (int k = 0; k < 3; ++k) CHECK(p[k] >= 1.8f && p[k] <= 2.3f);
    if (mode == VCY_DECIMATE_FIRST) CHECK(std::memcmp(p, crowd.v.data(), 3 * sizeof(float)) == 0);
  }

  // outputs that are not asked for; no faces, no vertices
  CHECK(decimate(open_patch, option(2.0f, -13.25f, VCY_DECIMATE_MEAN), &r, false, false) == VCY_OK && r.nv == 34 && r.nf == 47);
  CHECK(r.vmap[0] == 77 && r.src[0] == 77 && r.vn[0] == 77.0f && r.fn[0] == 77.0f);
  TestMesh lone;
  lone.v = {0.25f, -1.5f, 3.0f};
  CHECK(decimate(lone, option(2.0f, 0.0f, VCY_DECIMATE_MEAN), &r) == VCY_OK && r.nv == 0 && r.nf == 0 && r.vmap[0] == 77);
  {
    int64_t a = -1, b = -1;
    const vcy_decimate_option o = option(2.0f, 0.0f, 0);
    CHECK(vcy_decimate_mesh_host(0, 0, nullptr, nullptr, &o, nullptr, nullptr, &a, &b, nullptr, nullptr, nullptr, nullptr) == VCY_OK);
    CHECK(a == 0 && b == 0);
  }

  // refusals: nothing is written, not even the counts
  const auto refused = [&](const TestMesh& m, const vcy_decimate_option& o, int status) {
    return decimate(m, o, &r) == status && untouched(r);
  };
  CHECK(refused(oct, option(0.0f, 0.0f, 0), VCY_ERR_INVALID_ARG));
  CHECK(std::strstr(vcy::g_error, "cell") != nullptr);
  CHECK(refused(oct, option(-2.0f, 0.0f, 0), VCY_ERR_INVALID_ARG));
  CHECK(refused(oct, option(std::nanf(""), 0.0f, 0), VCY_ERR_INVALID_ARG));
  CHECK(refused(oct, option(INFINITY, 0.0f, 0), VCY_ERR_INVALID_ARG));
  CHECK(refused(oct, option(1.0f, std::nanf(""), 0), VCY_ERR_INVALID_ARG));
  CHECK(refused(oct, option(1.0f, -INFINITY, 0), VCY_ERR_INVALID_ARG));
  CHECK(refused(oct, option(1.0f, 0.0f, 3), VCY_ERR_INVALID_ARG));
  CHECK(refused(oct, option(1.0f, 0.0f, -1), VCY_ERR_INVALID_ARG));
  TestMesh bad = oct;
  bad.f[7] = 6;
  CHECK(refused(bad, option(1.0f, 0.0f, 0), VCY_ERR_INVALID_ARG));
  CHECK(std::strstr(vcy::g_error, "face 2") != nullptr);
  bad.f[7] = -1;
  CHECK(refused(bad, option(1.0f, 0.0f, 0), VCY_ERR_INVALID_ARG));
  bad = oct;
  bad.v[4] = std::nanf("");
  CHECK(refused(bad, option(1.0f, 0.0f, 0), VCY_ERR_INVALID_ARG));
  CHECK(std::strstr(vcy::g_error, "vertex 1") != nullptr);
  bad.v[4] = INFINITY;
  CHECK(refused(bad, option(1.0f, 0.0f, 0), VCY_ERR_INVALID_ARG));
  bad.v[4] = 1073741824.0f;  // |t| == 2^30 at cell 1
  CHECK(refused(bad, option(1.0f, 0.0f, 0), VCY_ERR_INVALID_ARG));
  bad.v[4] = -3.0e38f;       // p - origin overflows
  CHECK(refused(bad, option(1.0f, 3.0e38f, 0), VCY_ERR_INVALID_ARG));
  bad.v[4] = 1073741760.0f;  // the float below 2^30: fine
  CHECK(decimate(bad, option(1.0f, 0.0f, 0), &r) == VCY_OK && well_formed(bad, r));
  {
    const vcy_decimate_option o = option(1.0f, 0.0f, 0);
    int64_t a = -1, b = -1;
    std::vector<float> vo(oct.v.size(), 77.0f);
    std::vector<int32_t> fo(oct.f.size(), 77);
    CHECK(vcy_decimate_mesh_host(oct.nv(), (int64_t)1 << 30, oct.v.data(), oct.f.data(), &o, vo.data(), fo.data(), &a, &b, nullptr, nullptr, nullptr, nullptr) == VCY_ERR_UNSUPPORTED);
    CHECK(vcy_decimate_mesh_host((int64_t)1 << 31, oct.nf(), oct.v.data(), oct.f.data(), &o, vo.data(), fo.data(), &a, &b, nullptr, nullptr, nullptr, nullptr) == VCY_ERR_UNSUPPORTED);
    CHECK(vcy_decimate_mesh_host(oct.nv(), oct.nf(), oct.v.data(), oct.f.data(), nullptr, vo.data(), fo.data(), &a, &b, nullptr, nullptr, nullptr, nullptr) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_decimate_mesh_host(oct.nv(), oct.nf(), oct.v.data(), oct.f.data(), &o, nullptr, fo.data(), &a, &b, nullptr, nullptr, nullptr, nullptr) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_decimate_mesh_host(oct.nv(), oct.nf(), oct.v.data(), oct.f.data(), &o, vo.data(), nullptr, &a, &b, nullptr, nullptr, nullptr, nullptr) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_decimate_mesh_host(oct.nv(), oct.nf(), oct.v.data(), oct.f.data(), &o, vo.data(), fo.data(), nullptr, &b, nullptr, nullptr, nullptr, nullptr) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_decimate_mesh_host(oct.nv(), oct.nf(), oct.v.data(), oct.f.data(), &o, vo.data(), fo.data(), &a, nullptr, nullptr, nullptr, nullptr, nullptr) == VCY_ERR_INVALID_ARG);
    CHECK(vcy_decimate_mesh_host(-1, oct.nf(), oct.v.data(), oct.f.data(), &o, vo.data(), fo.data(), &a, &b, nullptr, nullptr, nullptr, nullptr) == VCY_ERR_INVALID_ARG);
    CHECK(a == -1 && b == -1 && vo[0] == 77.0f && fo[0] == 77);
  }

  std::puts("decimate_host_check: ok");
  return 0;
}
