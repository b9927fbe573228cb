// Vertex-clustering decimation of an indexed mesh, serially on the host (vcy_decimate_mesh_host; the definition is the
// section "mesh decimation" of vacancy_hip.h, restated in numpy in tests/decimate_ref.py).  Host code only -- no GPU, no
// context, nothing of the HIP runtime --, like mesh_smooth_host.hip; vcy_mesh_normals_host (mesh_host.hip) gives the
// normals of the result.  Also the argument checks the device entry point (mesh_decimate.hip) shares, and the same with
// quadric-error representatives (vcy_decimate_mesh_quadric_host; "mesh decimation, quadric representatives", restated in
// tests/quadric_ref.py; the arithmetic: mesh_quadric.h).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "mesh_decimate.h"
#include "mesh_quadric.h"
#include "host_shared.h"
#include "vacancy_hip.h"

namespace vcy {

void set_error(const char* fmt, ...);

// Everything the definition refuses without looking into the arrays, before anything is written.  `regularize`: non-NULL
// for the quadric entry points, whose rule (MEAN, a regularisation in [0, 1]) stands where the mode check does.
int decimate_check_args(const char* who, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                        const vcy_decimate_option* o, const float* vertices_out, const int32_t* faces_out,
                        const int64_t* n_vertices_out, const int64_t* n_faces_out, const float* regularize) {
  if (n_vertices < 0 || n_faces < 0 || !o || !n_vertices_out || !n_faces_out ||
      (n_vertices > 0 && n_faces > 0 && (!vertices || !faces || !vertices_out || !faces_out))) {
    set_error("%s: invalid argument", who);
    return VCY_ERR_INVALID_ARG;
  }
  if (!std::isfinite(o->cell) || !(o->cell > 0.0f)) {
    set_error("%s: cell %g must be finite and > 0", who, (double)o->cell);
    return VCY_ERR_INVALID_ARG;
  }
  if (!std::isfinite(o->origin[0]) || !std::isfinite(o->origin[1]) || !std::isfinite(o->origin[2])) {
    set_error("%s: the origin must be finite (%g, %g, %g)", who, (double)o->origin[0], (double)o->origin[1], (double)o->origin[2]);
    return VCY_ERR_INVALID_ARG;
  }
  if (regularize) {
    if (o->mode != VCY_DECIMATE_MEAN) {
      set_error("%s: mode %d: quadric representatives start from MEAN (0)", who, o->mode);
      return VCY_ERR_INVALID_ARG;
    }
    if (!std::isfinite(*regularize) || !(*regularize >= 0.0f) || !(*regularize <= 1.0f)) {
      set_error("%s: regularize %g must be finite and in [0, 1]", who, (double)*regularize);
      return VCY_ERR_INVALID_ARG;
    }
  } else if (o->mode < VCY_DECIMATE_MEAN || o->mode > VCY_DECIMATE_FIRST) {
    set_error("%s: mode %d outside 0 .. 2", who, o->mode);
    return VCY_ERR_INVALID_ARG;
  }
  { const int rc = mesh_index_limits(who, n_vertices, n_faces); if (rc != VCY_OK) return rc; }
  return VCY_OK;
}

}  // namespace vcy

using namespace vcy;

namespace {

// slots of an open-addressing table for n entries: a power of two >= 2 n
size_t table_slots(size_t n) {
  size_t s = 16;
  while (s < 2 * n) s <<= 1;
  return s;
}

// The definition, serially.  `regularize` non-NULL: MEAN with quadric representatives, and their fallbacks counted.
int decimate_host(const char* who, int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                  const vcy_decimate_option* option, const float* regularize, float* vertices_out, int32_t* faces_out,
                  int64_t* n_vertices_out, int64_t* n_faces_out, int32_t* vertex_map, int32_t* face_source,
                  float* vertex_normals_out, float* face_normals_out, int64_t* n_fallback) {
  { const int rc = decimate_check_args(who, n_vertices, n_faces, vertices, faces, option, vertices_out, faces_out, n_vertices_out, n_faces_out, regularize); if (rc != VCY_OK) return rc; }
  if (n_vertices == 0 || n_faces == 0) {
    *n_vertices_out = *n_faces_out = 0;
    if (n_fallback) *n_fallback = 0;
    return VCY_OK;
  }
  const size_t nv = (size_t)n_vertices, nf = (size_t)n_faces;
  for (size_t i = 0; i < 3 * nf; ++i)
    if (faces[i] < 0 || faces[i] >= n_vertices) {
      set_error("%s: face %lld names vertex %d of %lld", who, (long long)(i / 3), faces[i], (long long)n_vertices);
      return VCY_ERR_INVALID_ARG;
    }
  std::vector<int32_t> key(3 * nv);
  for (size_t v = 0; v < nv; ++v)
    if (!dc::cell_key(vertices + 3 * v, option->origin, option->cell, &key[3 * v])) {
      set_error("%s: vertex %lld (%g, %g, %g) is not finite or lies 2^30 cells or more from the origin", who, (long long)v,
                (double)vertices[3 * v], (double)vertices[3 * v + 1], (double)vertices[3 * v + 2]);
      return VCY_ERR_INVALID_ARG;
    }

  // clusters: vertices in ascending index through a table of representatives, so a cell's first vertex is its lowest member
  // and cluster numbers come out in the definition's order
  std::vector<int32_t> cluster(nv);  // cluster number of every vertex
  std::vector<int32_t> rep;          // lowest member of every cluster
  {
    const size_t slots = table_slots(nv), mask = slots - 1;
    std::vector<int32_t> table(slots, -1);
    for (size_t v = 0; v < nv; ++v) {
      const int32_t* k = &key[3 * v];
      size_t h = dc::hash3((uint32_t)k[0], (uint32_t)k[1], (uint32_t)k[2]) & mask;
      for (;; h = (h + 1) & mask) {
        const int32_t r = table[h];
        if (r < 0) {
          table[h] = (int32_t)v;
          cluster[v] = (int32_t)rep.size();
          rep.push_back((int32_t)v);
          break;
        }
        const int32_t* kr = &key[3 * (size_t)r];
        if (kr[0] == k[0] && kr[1] == k[1] && kr[2] == k[2]) {
          cluster[v] = cluster[(size_t)r];
          break;
        }
      }
    }
  }
  const size_t ncl = rep.size();

  // faces: corners -> cluster numbers, collapsed faces dropped, of the faces with one canonical form the first kept
  std::vector<int32_t> survivor;  // input indices, ascending
  std::vector<int32_t> out_id(ncl, -1);
  {
    const size_t slots = table_slots(nf), mask = slots - 1;
    std::vector<int32_t> table(slots, -1);
    std::vector<int32_t> canon(3 * nf);
    for (size_t f = 0; f < nf; ++f) {
      int32_t t[3] = {cluster[(size_t)faces[3 * f]], cluster[(size_t)faces[3 * f + 1]], cluster[(size_t)faces[3 * f + 2]]};
      if (t[0] == t[1] || t[1] == t[2] || t[2] == t[0]) continue;
      int32_t* c = &canon[3 * f];
      dc::canonical(t[0], t[1], t[2], c);
      size_t h = dc::hash3((uint32_t)c[0], (uint32_t)c[1], (uint32_t)c[2]) & mask;
      for (;; h = (h + 1) & mask) {
        const int32_t r = table[h];
        if (r < 0) {
          table[h] = (int32_t)f;
          survivor.push_back((int32_t)f);
          out_id[(size_t)t[0]] = out_id[(size_t)t[1]] = out_id[(size_t)t[2]] = 0;
          break;
        }
        const int32_t* cr = &canon[3 * (size_t)r];
        if (cr[0] == c[0] && cr[1] == c[1] && cr[2] == c[2]) break;  // a duplicate of the earlier face r
      }
    }
  }
  size_t nvo = 0;
  for (size_t c = 0; c < ncl; ++c)
    if (out_id[c] == 0) out_id[c] = (int32_t)nvo++;
  const size_t nfo = survivor.size();

  // member rows in ascending index behind off[c] (a counting sort is stable); FIRST needs none
  std::vector<int64_t> off;
  std::vector<int32_t> member;
  if (option->mode != VCY_DECIMATE_FIRST) {
    off.assign(ncl + 1, 0);
    for (size_t v = 0; v < nv; ++v) ++off[(size_t)cluster[v] + 1];
    for (size_t c = 0; c < ncl; ++c) off[c + 1] += off[c];
    member.resize(nv);
    std::vector<int64_t> cursor(off.begin(), off.end() - 1);
    for (size_t v = 0; v < nv; ++v) member[(size_t)cursor[(size_t)cluster[v]]++] = (int32_t)v;
  }

  // quadric representatives: corner rows 3 f + j in ascending order behind coff[v] (the same counting sort)
  std::vector<int64_t> coff;
  std::vector<int32_t> corner;
  if (regularize) {
    coff.assign(nv + 1, 0);
    for (size_t i = 0; i < 3 * nf; ++i) ++coff[(size_t)faces[i] + 1];
    for (size_t v = 0; v < nv; ++v) coff[v + 1] += coff[v];
    corner.resize(3 * nf);
    std::vector<int64_t> cursor(coff.begin(), coff.end() - 1);
    for (size_t i = 0; i < 3 * nf; ++i) corner[(size_t)cursor[(size_t)faces[i]]++] = (int32_t)i;
  }
  int64_t fallbacks = 0;

  // ---- nothing is refused past this point: the outputs
  for (size_t c = 0; c < ncl; ++c) {
    if (out_id[c] < 0) continue;
    size_t src = (size_t)rep[c];
    if (option->mode != VCY_DECIMATE_FIRST) {
      const int32_t* row = member.data() + off[c];
      const int64_t len = off[c + 1] - off[c];
      float m[3];
      dc::row_mean(vertices, row, len, m);
      if (regularize) {
        double Q[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int64_t j = 0; j < len; ++j) {  // (a vertex has one cluster: its Qv is needed here and nowhere else)
          const size_t v = (size_t)row[j];
          double Qv[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, q[9];
          for (int64_t k = coff[v]; k < coff[v + 1]; ++k) {
            const int32_t* tri = faces + 3 * (size_t)(corner[(size_t)k] / 3);
            dc::face_quadric(vertices + 3 * (size_t)tri[0], vertices + 3 * (size_t)tri[1], vertices + 3 * (size_t)tri[2], m, q);
            dc::quadric_add(Qv, q);
          }
          dc::quadric_add(Q, Qv);
        }
        float P[3];
        if (dc::solve_or_mean(Q, m, *regularize, option->origin, option->cell, &key[3 * (size_t)rep[c]], P)) ++fallbacks;
        std::memcpy(vertices_out + 3 * (size_t)out_id[c], P, 3 * sizeof(float));
        continue;
      }
      if (option->mode == VCY_DECIMATE_MEAN) {
        std::memcpy(vertices_out + 3 * (size_t)out_id[c], m, 3 * sizeof(float));
        continue;
      }
      src = (size_t)dc::row_nearest(vertices, row, len, m);
    }
    std::memcpy(vertices_out + 3 * (size_t)out_id[c], vertices + 3 * src, 3 * sizeof(float));  // (memcpy: the input bits)
  }
  for (size_t g = 0; g < nfo; ++g) {
    const size_t f = (size_t)survivor[g];
    for (int j = 0; j < 3; ++j) faces_out[3 * g + j] = out_id[(size_t)cluster[(size_t)faces[3 * f + j]]];
    if (face_source) face_source[g] = (int32_t)f;
  }
  if (vertex_map)
    for (size_t v = 0; v < nv; ++v) vertex_map[v] = out_id[(size_t)cluster[v]];
  *n_vertices_out = (int64_t)nvo;
  *n_faces_out = (int64_t)nfo;
  if (n_fallback) *n_fallback = fallbacks;
  if (vertex_normals_out || face_normals_out)
    return vcy_mesh_normals_host((int64_t)nvo, (int64_t)nfo, vertices_out, faces_out, vertex_normals_out, face_normals_out);
  return VCY_OK;
}

}  // namespace

extern "C" {

int vcy_decimate_mesh_host(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                           const vcy_decimate_option* option, float* vertices_out, int32_t* faces_out,
                           int64_t* n_vertices_out, int64_t* n_faces_out, int32_t* vertex_map, int32_t* face_source,
                           float* vertex_normals_out, float* face_normals_out) {
  return decimate_host("vcy_decimate_mesh_host", n_vertices, n_faces, vertices, faces, option, nullptr, vertices_out, faces_out,
                       n_vertices_out, n_faces_out, vertex_map, face_source, vertex_normals_out, face_normals_out, nullptr);
}

int vcy_decimate_mesh_quadric_host(int64_t n_vertices, int64_t n_faces, const float* vertices, const int32_t* faces,
                                   const vcy_decimate_option* option, float regularize, float* vertices_out, int32_t* faces_out,
                                   int64_t* n_vertices_out, int64_t* n_faces_out, int32_t* vertex_map, int32_t* face_source,
                                   float* vertex_normals_out, float* face_normals_out, int64_t* n_fallback) {
  return decimate_host("vcy_decimate_mesh_quadric_host", n_vertices, n_faces, vertices, faces, option, &regularize, vertices_out,
                       faces_out, n_vertices_out, n_faces_out, vertex_map, face_source, vertex_normals_out, face_normals_out,
                       n_fallback);
}

}  // extern "C"
