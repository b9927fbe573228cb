// The mesh operators on meshes that are in device memory already: the middle parts of vcy_smooth_mesh (mesh_smooth.hip)
// and vcy_decimate_mesh[_quadric] (mesh_decimate.hip), between "bring the input into the pool" and "copy out".  The two
// entry points are these with a host-to-device copy in front and the copies into the caller's arrays behind; the extraction
// chain (mesh_chain.hip) runs them on the staged mesh of the extraction.  Everything goes to the context's stream.
#pragma once

#include "mesh_rows.h"
#include "vcy_internal.h"

namespace vcy {

// ---- smoothing ---------------------------------------------------------------------------------------------------
// Where a mesh that is on the device already comes from.  `table`: the vertex -> incident-corner table of `faces`, counted,
// scanned and filled (rows::fill; the rows in any order) by the caller in memory of its own: the smoothing sorts its rows
// and leaves them sorted.
struct SmoothInput {
  const float* vertices;  // [3 n] copied into the pool (the passes write their positions)
  const int32_t* faces;   // [3 nf] read in place
  const rows::Table* table;
};
struct SmoothResult {  // in the smoothing's pool (vcy_ctx::d_sm_buf) until the context next smooths
  const float* vertices;
  const float* face_normals;    // null unless normals were asked for
  const float* vertex_normals;  // null unless asked for
};
// `host_vertices` / `host_faces`: the caller's arrays (vcy_smooth_mesh), `in` null; or `in`, the two null.  Launches the
// table (unless given), the passes and the normals; waits for nothing; vcy_ctx::ev_sm[0 .. 3] lie around the three groups.
int smooth_launch(vcy_ctx* c, int64_t n, int64_t nf, const float* host_vertices, const int32_t* host_faces, const SmoothInput* in,
                  const vcy_smooth_option& o, bool vertex_normals, bool face_normals, SmoothResult* res);
// after a wait for the stream: vcy_ctx::last_smooth_ms
int smooth_read_times(vcy_ctx* c, bool normals);

// ---- decimation --------------------------------------------------------------------------------------------------
// `coff` / `corner`: offsets and rows of the vertex -> incident-corner table of `faces` (quadric representatives), filled,
// rows in any order or sorted; null: the decimation builds its own.
struct DecimateInput {
  const float* vertices;  // [3 n] read in place
  const int32_t* faces;   // [3 nf] read in place
  int* coff;
  int* corner;
};
struct DecimateResult {  // in the decimation's pool (vcy_ctx::d_dc_buf) and the normals' (d_mn_buf) until the context next decimates
  int64_t n_vertices, n_faces, n_fallback;
  const float* vertices;
  const int32_t* faces;
  const int32_t* vertex_map;   // [n]
  const int32_t* face_source;  // [n_faces]
  const float* face_normals;    // null unless normals were asked for and n_faces > 0
  const float* vertex_normals;  // null unless asked for and n_faces > 0
};
// `host_vertices` / `host_faces` or `in`, as above.  Launches the three groups, WAITS for their flags and counts (the one
// wait of a decimation), then launches the normals of the output mesh.  `regularize` non-null: quadric representatives.
int decimate_launch(const char* who, vcy_ctx* c, int64_t n, int64_t nf, const float* host_vertices, const int32_t* host_faces,
                    const DecimateInput* in, const vcy_decimate_option& o, const float* regularize, bool vertex_normals,
                    bool face_normals, DecimateResult* res);
// after a wait for the stream: vcy_ctx::last_decimate_ms, last_quadric_ms
int decimate_read_times(vcy_ctx* c, bool normals, bool quadric);

}  // namespace vcy
