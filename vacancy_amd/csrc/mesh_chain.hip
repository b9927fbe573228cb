// The extraction chain, vcy_extract_iso_chain: extract, smooth, decimate and normals in one call, the mesh staying in
// device memory between the stages (the definition: the section "extraction chain" of vacancy_hip.h).
//
// No kernel in this file: the stages are the launches of the separate calls on the arrays the stage before has left.
//   extract  extract_iso_staged (mc_extract.hip): the mesh in vcy_ctx::d_mc_out, float vertices and int faces; the counts
//            come from the extraction's own single wait (two when a capacity guess was too small).
//   table    the vertex -> incident-corner table of the extracted mesh: mesh_rows.h's count, scan and fill over the staged
//            faces or, "chainrows" 1, mc_corner_rows over the extraction's cells (mc_normals.hip), in a pool of the
//            chain's own (vcy_ctx::d_ch_buf) -- so it outlives the decimation's member table, which in
//            vcy_decimate_mesh_quadric shares counts and cursors with the corner table.  Built when the smoothing or the
//            quadric stage runs, once: smoothing moves vertices, not faces.
//   smooth   smooth_launch (mesh_smooth.hip) sorts the table's rows, writes its gather rows and runs the passes on a
//            device-to-device copy of the positions; the faces are read in place.  Without a decimation its normals, through
//            the same table, are the result's.
//   decimate decimate_launch (mesh_decimate.hip) on the smoothed positions (or the staged ones) and the staged faces, both
//            in place; dc_qv reads the chain's table (sorting a sorted row changes nothing).  It waits for its flags and
//            counts -- the chain's second wait -- and launches the normals of its output.
//   output   page-locked host arrays of the library's pool, sized by the final counts; the copies, and the third wait.
// The face indices are the library's own and are not checked on the way (the table is filled by the unchecked kernels); the
// check of the vertex cell rule stays, inside the decimation.
#include <chrono>
#include <cstring>

#include "mc_common.h"
#include "mesh_ops.h"
#include "mesh_rows.h"
#include "vcy_internal.h"

namespace vcy {

namespace {

enum { kMsExtract, kMsTable, kMsPasses, kMsCluster, kMsQuadric, kMsFacesEmit, kMsNormals, kMsWall };

// the option's refusals: those of the separate calls, by their own checks on a mesh of no elements
int chain_check_option(const char* who, const vcy_chain_option* o) {
  if (!o || (o->smooth != 0 && o->smooth != 1) || o->decimate < 0 || o->decimate > 2 || (o->maps != 0 && o->maps != 1) ||
      (o->which & ~(VCY_NORMALS_VERTEX | VCY_NORMALS_FACE)) != 0) {
    set_error("%s: invalid argument", who);
    return VCY_ERR_INVALID_ARG;
  }
  if (o->smooth) {
    const int rc = smooth_check_args(who, 0, 0, nullptr, nullptr, &o->smooth_option, nullptr);
    if (rc != VCY_OK) return rc;
  }
  if (o->decimate) {
    int64_t none = 0;
    const int rc = decimate_check_args(who, 0, 0, nullptr, nullptr, &o->decimate_option, nullptr, nullptr, &none, &none,
                                       o->decimate == 2 ? &o->regularize : nullptr);
    if (rc != VCY_OK) return rc;
  }
  return VCY_OK;
}

// `count` elements of `bytes_each` from the device into a fresh array of the host pool, queued on the stream
template <typename T>
int to_host(hipStream_t s, T** dst, const T* src, size_t count, size_t per) {
  *dst = (T*)mesh_host_alloc(sizeof(T) * per * count);
  if (!*dst) {
    set_error("out of host memory for the mesh");
    return VCY_ERR_INTERNAL;
  }
  VCY_HIP_CHECK(hipMemcpyAsync(*dst, src, sizeof(T) * per * count, hipMemcpyDeviceToHost, s));
  return VCY_OK;
}

int chain_device(vcy_ctx* c, double iso, int linear_interp, const vcy_chain_option& o, vcy_mesh* out, vcy_mesh_normals* normals,
                 vcy_chain_report* report) {
  hipStream_t s = c->stream;
  float* ms = c->last_chain_ms;
  { const int rc = materialize(c); if (rc != VCY_OK) return rc; }
  StagedMesh m{};
  { const int rc = extract_iso_staged(c, iso, linear_interp, &m); if (rc != VCY_OK) return rc; }
  ms[kMsExtract] = c->last_extract_device_ms;
  if (report) report->n_extracted_vertices = m.n_vertices, report->n_extracted_faces = m.n_faces;
  if (m.n_vertices == 0 || m.n_faces == 0) return VCY_OK;  // (an empty mesh: every stage returns it as it is)
  // (the size the separate calls refuse -- their tables hold 32-bit vertex and corner ids, and so do the chain's; the
  // extraction itself goes further -- with their code, before anything is launched on the mesh)
  { const int rc = mesh_index_limits("vcy_extract_iso_chain", m.n_vertices, m.n_faces); if (rc != VCY_OK) return rc; }
  const size_t n = (size_t)m.n_vertices, nf = (size_t)m.n_faces, nc = 3 * nf;
  const bool quadric = o.decimate == 2;
  const bool want_vn = (o.which & VCY_NORMALS_VERTEX) != 0, want_fn = (o.which & VCY_NORMALS_FACE) != 0;

  // ---- the one table: [deg, scan scratch, total | off | cursor | corners]
  rows::Table t{};
  const bool table = o.smooth || quadric;
  if (table) {
    const bool from_cells = c->chain_rows != 0;
    PoolLayout at;
    const size_t at_deg = at.take(8 * (n + 1)), at_scan = at.take(8 * scan_scratch_words(n + 1)), at_total = at.take(8),
                 at_off = at.take(4 * (n + 1)), at_cursor = at.take(4 * n), at_corners = at.take(4 * nc),
                 at_fbase = at.take(from_cells ? 4 * (size_t)m.cells.n_cells : 0);
    VCY_HIP_CHECK(c->d_ch_buf.grow(at.total(), s));
    char* base = (char*)c->d_ch_buf;
    t = rows::Table{(int)n, (int)nc, m.faces, (rows::u64*)(base + at_deg), (int*)(base + at_off), (int*)(base + at_cursor),
                    (int*)(base + at_corners)};
    for (vcy::Event& e : c->ev_ch) VCY_HIP_CHECK(e.ensure());
    VCY_HIP_CHECK(hipEventRecord(c->ev_ch[0], s));
    if (from_cells) {  // "chainrows" 1: counts and rows from the cells, every row ascending as it is written
      mc::CornerRowsLaunch a = m.cells;
      a.face_base = (uint32_t*)(base + at_fbase), a.deg = t.deg, a.off = t.off, a.items = t.items;
      VCY_HIP_CHECK(hipMemsetAsync(t.deg, 0, 8 * (n + 1), s));
      VCY_HIP_CHECK(mc::launch_corner_rows_count(s, m.p, a));
      { const int rc = device_exclusive_scan_u64(t.deg, (int64_t)n + 1, (rows::u64*)(base + at_total), (rows::u64*)(base + at_scan), s); if (rc != VCY_OK) return rc; }
      hipLaunchKernelGGL(rows::rows_offsets_kernel, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, s, t);
      VCY_HIP_CHECK(mc::launch_corner_rows_fill(s, m.p, a));
    } else {
      const int rc = rows::fill(s, t, (rows::u64*)(base + at_total), (rows::u64*)(base + at_scan));
      if (rc != VCY_OK) return rc;
    }
    VCY_HIP_CHECK(hipEventRecord(c->ev_ch[1], s));
  }

  // ---- the stages
  const float* pos = m.vertices;
  SmoothResult sr{};
  if (o.smooth) {
    const SmoothInput in{m.vertices, m.faces, &t};
    const bool last = o.decimate == 0;  // (its normals are the result's)
    const int rc = smooth_launch(c, m.n_vertices, m.n_faces, nullptr, nullptr, &in, o.smooth_option, last && want_vn, last && want_fn, &sr);
    if (rc != VCY_OK) return rc;
    pos = sr.vertices;
  }
  DecimateResult dr{};
  if (o.decimate) {
    const DecimateInput in{pos, m.faces, quadric ? t.off : nullptr, quadric ? t.items : nullptr};
    const int rc = decimate_launch("vcy_extract_iso_chain", c, m.n_vertices, m.n_faces, nullptr, nullptr, &in, o.decimate_option,
                                   quadric ? &o.regularize : nullptr, want_vn, want_fn, &dr);  // (waits: flags and counts)
    if (rc != VCY_OK) return rc;
  }

  // ---- the output: sized by the final counts, copied, waited for
  const size_t nvo = o.decimate ? (size_t)dr.n_vertices : n, nfo = o.decimate ? (size_t)dr.n_faces : nf;
  const float* d_v = o.decimate ? dr.vertices : pos;
  const int32_t* d_f = o.decimate ? dr.faces : m.faces;
  const float* d_vn = o.decimate ? dr.vertex_normals : sr.vertex_normals;
  const float* d_fn = o.decimate ? dr.face_normals : sr.face_normals;
  int rc = VCY_OK;
  if (nfo > 0) {
    rc = to_host(s, &out->vertices, d_v, nvo, 3);
    if (rc == VCY_OK) rc = to_host(s, &out->faces, d_f, nfo, 3);
    if (rc == VCY_OK && want_vn && d_vn) rc = to_host(s, &normals->vertex_normals, d_vn, nvo, 3);
    if (rc == VCY_OK && want_fn && d_fn) rc = to_host(s, &normals->face_normals, d_fn, nfo, 3);
    if (rc == VCY_OK && report && o.maps && o.decimate) rc = to_host(s, &report->face_source, dr.face_source, nfo, 1);
  }
  if (rc == VCY_OK && report && o.maps && o.decimate) rc = to_host(s, &report->vertex_map, dr.vertex_map, n, 1);
  if (rc != VCY_OK) return rc;
  VCY_HIP_CHECK(hipStreamSynchronize(s));
  if (nfo > 0) out->n_vertices = (int64_t)nvo, out->n_faces = (int64_t)nfo;
  if (report) report->n_fallback = dr.n_fallback;

  // ---- times
  if (table) VCY_HIP_CHECK(hipEventElapsedTime(&ms[kMsTable], c->ev_ch[0], c->ev_ch[1]));
  if (o.smooth) {
    { const int rc2 = smooth_read_times(c, o.decimate == 0 && o.which != 0); if (rc2 != VCY_OK) return rc2; }
    ms[kMsTable] += c->last_smooth_ms[0];
    ms[kMsPasses] = c->last_smooth_ms[1];
    ms[kMsNormals] = c->last_smooth_ms[2];
  }
  if (o.decimate) {
    { const int rc2 = decimate_read_times(c, o.which != 0, quadric); if (rc2 != VCY_OK) return rc2; }
    ms[kMsCluster] = c->last_decimate_ms[0];
    ms[kMsQuadric] = quadric ? c->last_quadric_ms : 0.0f;
    ms[kMsFacesEmit] = c->last_decimate_ms[1] + c->last_decimate_ms[2];
    ms[kMsNormals] = c->last_decimate_ms[3];
  }
  return VCY_OK;
}

}  // namespace

}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_extract_iso_chain(vcy_ctx* c, double iso, int linear_interp, const vcy_chain_option* option, vcy_mesh* out,
                          vcy_mesh_normals* normals, vcy_chain_report* report) {
  const char* who = "vcy_extract_iso_chain";
  { const int rc = chain_check_option(who, option); if (rc != VCY_OK) return rc; }
  if (!out || (!normals && option->which != 0)) {
    set_error("%s: invalid argument", who);
    return VCY_ERR_INVALID_ARG;
  }
  std::memset(out, 0, sizeof(*out));
  if (normals) std::memset(normals, 0, sizeof(*normals));
  if (report) std::memset(report, 0, sizeof(*report));
  if (!c) {  // (behind the argument checks: those need no context)
    set_error("voxel grid has not been initialized");
    return VCY_ERR_NOT_INITIALIZED;
  }
  for (float& ms : c->last_chain_ms) ms = 0.0f;  // (a call refused below reports no times, not the last call's)
  if (c->z0 != 0 || c->z1 != c->nz || c->halo_lo != 0) {
    set_error("%s: the context owns z [%d, %d) of %d slices; a slab's mesh is a part, and the merged mesh exists only on the "
              "host (merge the slabs' meshes, then vcy_smooth_mesh / vcy_decimate_mesh)", who, c->z0, c->z1, c->nz);
    return VCY_ERR_UNSUPPORTED;
  }
  if (c->mesh_keys) {
    set_error("%s: the context returns edge keys, which the chain's mesh has not (vcy_set_param \"meshkeys\" 0)", who);
    return VCY_ERR_UNSUPPORTED;
  }
  VCY_HIP_CHECK(hipSetDevice(c->device));
  const auto t0 = std::chrono::steady_clock::now();
  int rc;
  if (!option->smooth && !option->decimate) {  // vcy_extract_iso_normals, by definition
    rc = option->which ? vcy_extract_iso_normals(c, iso, linear_interp, option->which, out, normals) : vcy_extract_iso(c, iso, linear_interp, out);
    if (rc == VCY_OK) {
      c->last_chain_ms[kMsExtract] = c->last_extract_device_ms;
      c->last_chain_ms[kMsNormals] = c->last_normals_device_ms;
      if (report) report->n_extracted_vertices = out->n_vertices, report->n_extracted_faces = out->n_faces;
    }
  } else {
    rc = chain_device(c, iso, linear_interp, *option, out, normals, report);
    if (rc != VCY_OK) {
      (void)hipStreamSynchronize(c->stream);  // (queued copies still name the arrays released below)
      vcy_mesh_free(out);
      if (normals) vcy_mesh_normals_free(normals);
      if (report) vcy_chain_report_free(report);
    }
  }
  c->last_chain_ms[kMsWall] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

int vcy_mesh_index_limits(int64_t n_vertices, int64_t n_faces) {
  if (n_vertices < 0 || n_faces < 0) {
    set_error("vcy_mesh_index_limits: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  return mesh_index_limits("vcy_mesh_index_limits", n_vertices, n_faces);
}

void vcy_chain_report_free(vcy_chain_report* r) {
  if (!r) return;
  mesh_host_free(r->vertex_map);
  mesh_host_free(r->face_source);
  r->vertex_map = nullptr, r->face_source = nullptr;
}

int vcy_last_chain_ms(const vcy_ctx* c, float* extract_ms, float* table_ms, float* passes_ms, float* cluster_ms, float* quadric_ms,
                      float* faces_emit_ms, float* normals_ms, float* wall_ms) {
  if (!c) return VCY_ERR_INVALID_ARG;
  float* outs[8] = {extract_ms, table_ms, passes_ms, cluster_ms, quadric_ms, faces_emit_ms, normals_ms, wall_ms};
  for (int k = 0; k < 8; ++k)
    if (outs[k]) *outs[k] = c->last_chain_ms[k];
  return VCY_OK;
}

}  // extern "C"
