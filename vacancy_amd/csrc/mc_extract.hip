// The host driver of the marching-cubes extraction, extract_iso() (kernels and launches: mc_kernels.hip, mc_normals.hip).
// How much the chain produces is data: the number of active cells sizes the list and the owner info, the numbers of
// vertices and triangles the output arrays.  The kernels read those counts from device memory, so with the sizes of
// this context's previous extraction as a guess (plus a quarter) the whole chain is enqueued without the host reading
// anything back; the counts are fetched once at the end, and if a guess was too small the chain runs again with the
// exact sizes -- which is also the path of the first extraction.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>

#include "mc_common.h"
#include "vcy_internal.h"

namespace vcy {

using namespace mc;

namespace {

int64_t with_headroom(int64_t v) { return v + v / 4 + 4096; }  // the next view's mesh is a little different
double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The one owner of the host arrays in *out and *normals while an extraction runs.  Unless disarmed on success, its
// destructor leaves both structs empty and the arrays back in the pool -- after waiting for the stream when mc_emit
// has been pointed at them (`direct`) and may still be writing: the pool is shared, and the next mesh that takes
// these buffers must not receive this one's bytes.
struct HostMeshGuard {
  vcy_mesh* out;
  vcy_mesh_normals* normals;  // may be null
  hipStream_t stream;
  bool direct = false;  // out's arrays are the target of an enqueued mc_emit
  bool armed = true;

  void release_mesh() {  // (a guess that was too small, an empty mesh, a failed allocation)
    mesh_host_free(out->vertices);
    mesh_host_free(out->faces);
    mesh_host_free(out->edge_keys);
    out->vertices = nullptr, out->faces = nullptr, out->edge_keys = nullptr;
    direct = false;
  }
  ~HostMeshGuard() {
    if (!armed) return;
    if (direct) (void)hipStreamSynchronize(stream);  // best effort: there is no better place to report a failure
    release_mesh();
    out->n_vertices = out->n_faces = out->n_foreign_vertices = 0;
    if (normals) {
      mesh_host_free(normals->vertex_normals);
      mesh_host_free(normals->face_normals);
      normals->vertex_normals = nullptr, normals->face_normals = nullptr;
    }
  }
};

FastDiv make_div(uint32_t d) {
  FastDiv f;
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;  // ceil(log2 d)
  f.d = d;
  f.m = (uint32_t)((((1ull << l) - d) << 32) / d + 1);
  f.s1 = l < 1 ? l : 1;
  f.s2 = l < 1 ? 0 : l - 1;
  return f;
}

constexpr int64_t kFromTotals = -1;  // run_chain: size the output arrays from the totals the owner pass leaves

struct Extraction {
  vcy_ctx* c;
  hipStream_t s;
  vcy_mesh* out;
  int which;  // VCY_NORMALS_*
  vcy_mesh_normals* normals_out;
  int64_t* layer_faces;
  HostMeshGuard host;

  McParams p{};
  SweepParams q{};
  ChainLaunch chain{};  // (its buffers: scratch(), cell_buffers(), output_buffers())
  float *d_vn = nullptr, *d_fn = nullptr;
  volatile u64* report = nullptr;
  bool end_recorded = false, normals_timed = false;
  // number of active cells and what they produce
  int64_t ncells = 0, nv = 0, nf = 0, nforeign = 0, first_layer_faces = 0, last_layer_faces = 0;
  StagedMesh* staged = nullptr;  // extract_iso_staged: the mesh stays in the device staging, nothing is delivered
  bool timing = false;
  double t_begin = 0.0, t_ph[5] = {0, 0, 0, 0, 0};

  Extraction(vcy_ctx* ctx, vcy_mesh* o, int w, vcy_mesh_normals* n, int64_t* lf)
      : c(ctx), s(ctx->stream), out(o), which(n ? w : 0), normals_out(n), layer_faces(lf), host{o, n, ctx->stream} {}

  bool wants_normals() const { return which != 0 || layer_faces != nullptr; }
  ChainedScanSlot scan_slot(int k) {  // {flags, ticket, tickets_drawn, epoch} of slot k
    uint32_t* f = (uint32_t*)c->d_mc_flags;
    return {f + k * kChainedScanMaxChunks, f + 2 * kChainedScanMaxChunks + k, &c->mc_scan_tickets[k], ++c->mc_scan_epoch};
  }

  // The cell-word layout (McParams, mc_common.h), the sweep's geometry when it is taken, and the launch limits.
  int plan(double iso, int linear_interp, bool* any_cells) {
    p.sdf = c->d_sdf;
    p.cnt = c->d_cnt;
    p.px = c->d_px;
    p.py = c->d_py;
    p.pz = c->d_pz;
    p.nx = c->nx;
    p.ny = c->ny;
    p.nslices = c->halo_lo + c->nz_local();
    p.Wr = (c->nx + 63) / 64;
    p.Y = c->ny - 1;
    p.zc0 = std::max(c->z0, 1);
    p.L = c->z1 - p.zc0;
    p.zs0 = c->z0 - c->halo_lo;
    p.has_ghost = c->halo_lo > 0 ? 1 : 0;
    p.iso = iso;
    p.linear = linear_interp;
    c->last_extract_device_ms = 0.0f;
    c->last_normals_device_ms = 0.0f;
    if (layer_faces) layer_faces[0] = layer_faces[1] = 0;
    *any_cells = !(c->nx < 2 || p.Y <= 0 || p.L <= 0);  // no cells: the reference's loops do not run
    if (!*any_cells) return VCY_OK;
    // (the sweep needs a voxel row that is a power-of-two number of whole words; taken only on request, see launch_sweep)
    const bool sweep = c->mc_sweep && c->nx == p.Wr * 64 && (p.Wr & (p.Wr - 1)) == 0 && p.Wr <= 32;
    p.Yc = p.Y;
    if (sweep) {
      q.R = std::max(32, kWordsPerBlock / p.Wr);
      q.K = q.R * p.Wr / kWordsPerBlock;  // <= kSweepMaxK
      p.Yc = (p.Y + q.R - 1) / q.R * q.R;
      q.groups = p.Yc / q.R;
      // enough workgroups to fill the GPU, few enough that the slice two z chunks share stays a small part
      const int64_t want = ((int64_t)(p.L + 1) * q.groups + VCY_SWEEP_TARGET_WGS - 1) / VCY_SWEEP_TARGET_WGS;
      q.layers = (int)std::min<int64_t>(std::max<int64_t>(want, 8), 64);
      q.dl = p.zs0 - p.zc0 + 1;
      q.cnt_slices = c->st.cnt_implied ? 0 : p.nslices;
      while ((1 << q.wshift) < p.Wr) ++q.wshift;
      chain.sweep = &q;
    }
    const int64_t ghost_words = (int64_t)p.Yc * p.Wr;
    p.G = (ghost_words + kWordsPerBlock - 1) / kWordsPerBlock * kWordsPerBlock;
    p.nwords = p.G + (int64_t)p.L * p.Yc * p.Wr;
    p.small32 = p.nwords < 0xffffffffLL && (int64_t)p.Yc * p.Wr < 0x7fffffffLL ? 1 : 0;
    p.div_row = make_div((uint32_t)p.Wr);
    p.div_layer = make_div(p.small32 ? (uint32_t)((int64_t)p.Yc * p.Wr) : 1u);
    const int64_t nblocks64 = (p.nwords + kWordsPerBlock - 1) / kWordsPerBlock;
    const int64_t vox_words = (int64_t)p.nslices * c->ny * p.Wr;
    if (nblocks64 > 0x7fffffffLL || (vox_words + 3) / 4 > 0x7fffffffLL) {
      set_error("too many cells for one launch");
      return VCY_ERR_TOO_MANY_VOXELS;
    }
    chain.nblocks = (unsigned)nblocks64;
    return VCY_OK;
  }

  // What the context keeps for its extractions, made or grown on demand: the case tables, the scratch of the cell
  // search, the scans' publication flags, the event pair and the report block.
  int scratch() {
    if (!c->d_mc_tables) {
      McTables h;
      build_tables(&h);
      VCY_HIP_CHECK(c->d_mc_tables.alloc(sizeof(McTables)));
      VCY_HIP_CHECK(hipMemcpy(c->d_mc_tables, &h, sizeof(McTables), hipMemcpyHostToDevice));
    }
    chain.T = (const McTables*)c->d_mc_tables;

    // bit planes, ACT, per-word offsets, block counts (3 bits per voxel + 12.5 B per 64 cells: 0.9 GB at 1024^3)
    const bool sweep = chain.sweep != nullptr;
    const unsigned nblocks = chain.nblocks;
    const size_t sz_plane = align256(sizeof(u64) * (size_t)p.nslices * c->ny * p.Wr);
    const size_t sz_act = align256(sizeof(u64) * (size_t)p.nwords);
    const size_t sz_woff = align256(sizeof(uint32_t) * (size_t)p.nwords);
    const size_t sz_counts = align256(sizeof(u64) * ((size_t)nblocks + 1));
    const size_t sz_scan = align256(sizeof(u64) * scan_scratch_words((size_t)nblocks));
    const size_t sz_ghost = sweep ? align256(sizeof(u64) * 3 * (size_t)c->ny * p.Wr) : 0;  // IN / OK / TC of one slice
    const size_t need = (sweep ? 1 : 3) * sz_plane + sz_ghost + sz_act + sz_woff + sz_counts + sz_scan + 256;
    VCY_HIP_CHECK(c->d_mc_scratch.grow(need, s));
    char* base = (char*)c->d_mc_scratch;
    chain.in = (u64*)base;                     base += sz_plane;
    chain.ok = (u64*)base;                     base += sweep ? 0 : sz_plane;  // (the sweep keeps OK / TC in LDS)
    chain.tc = (u64*)base;                     base += sweep ? 0 : sz_plane;
    chain.ghost = (u64*)base;                  base += sz_ghost;
    chain.act = (u64*)base;                    base += sz_act;
    chain.word_cell_off = (uint32_t*)base;     base += sz_woff;
    chain.block_cells = (u64*)base;            base += sz_counts;
    chain.scan_scratch = (u64*)base;           base += sz_scan;
    chain.ncells_dev = (u64*)base;
    // publication flags of the chained scans (scan_chained_kernel): an allocation of their own, zeroed once -- they
    // must never hold a FUTURE epoch, so they do not live in scratch whose layout changes with the extraction
    if (!c->d_mc_flags) {
      // [2 slots][kChainedScanMaxChunks] flags, then the two ticket counters
      const size_t fbytes = sizeof(uint32_t) * (2 * (size_t)kChainedScanMaxChunks + 2);
      VCY_HIP_CHECK(c->d_mc_flags.alloc(fbytes));
      VCY_HIP_CHECK(hipMemsetAsync(c->d_mc_flags, 0, fbytes, s));
      c->mc_scan_epoch = 0;
      c->mc_scan_tickets[0] = c->mc_scan_tickets[1] = 0;
    }
    // the extraction has its own event pair: vcy_timer_begin / _end may bracket it
    VCY_HIP_CHECK(c->ev_mc_begin.ensure());
    VCY_HIP_CHECK(c->ev_mc_end.ensure());
    // The counts come back through 64 bytes of page-locked memory that mc_emit writes itself (see the kernel).
    if (!c->h_mc_report) {
      VCY_HIP_CHECK(c->h_mc_report.alloc(64));  // (portable + mapped: vcy_ctx::h_mc_report)
      std::memset((void*)c->h_mc_report, 0, 64);
    }
    report = (volatile u64*)c->h_mc_report;
    return VCY_OK;
  }

  int find_cells() {
    VCY_HIP_CHECK(hipEventRecord(c->ev_mc_begin, s));
    return launch_cell_search(c, &p, chain, scan_slot(0));
  }

  // the per-active-cell arrays, cached in the context
  int cell_buffers(int64_t cap_cells) {
    chain.cap_cells = cap_cells;
    chain.cell_blocks = (unsigned)((cap_cells + 255) / 256);
    const size_t sz_list = align256(sizeof(u64) * (size_t)cap_cells);
    const size_t sz_info = align256(sizeof(uint32_t) * (size_t)cap_cells);
    const size_t sz_nact = align256(sizeof(uint16_t) * (size_t)cap_cells);
    const size_t sz_cc = align256(sizeof(u64) * ((size_t)chain.cell_blocks + 1));
    const size_t sz_cs = align256(sizeof(u64) * scan_scratch_words((size_t)chain.cell_blocks));
    const size_t need = sz_list + sz_info + sz_nact + sz_cc + sz_cs + 256;
    VCY_HIP_CHECK(c->d_mc_cells.grow(need, s));
    char* b = (char*)c->d_mc_cells;
    chain.cell_list = (u64*)b;             b += sz_list;
    chain.info = (uint32_t*)b;             b += sz_info;
    chain.nbr_active = (uint16_t*)b;       b += sz_nact;
    chain.block_offs = (u64*)b;            b += sz_cc;
    chain.cell_scan_scratch = (u64*)b;     b += sz_cs;
    chain.grand_total_dev = (u64*)b;
    return VCY_OK;
  }

  // Where mc_emit writes: the page-locked host arrays the caller receives when the mesh is small enough ("mcdirect",
  // see launch_emit), else the device staging cached in the context.
  int output_buffers(int64_t cap_v, int64_t cap_f) {
    chain.cap_verts = cap_v;
    chain.cap_faces = cap_f;
    chain.report = (u64*)c->h_mc_report;
    const size_t sz_v = align256(sizeof(float) * 3 * (size_t)std::max<int64_t>(cap_v, 1));
    const size_t sz_k = align256(sizeof(long long) * 2 * (size_t)std::max<int64_t>(cap_v, 1));
    const size_t sz_f = align256(sizeof(int) * 3 * (size_t)std::max<int64_t>(cap_f, 1));
    // (with normals the mesh is staged on the device: mc_face_normals reads the emitted arrays, and must not read them
    // back over PCIe)
    if (!wants_normals() && !staged && (int64_t)(sz_v + sz_f + (c->mesh_keys ? sz_k : 0)) <= c->mc_direct_bytes) {
      bool pinned = true, pk = true, pf = true;
      out->vertices = (float*)mesh_host_alloc(sz_v, &pinned);
      out->faces = (int32_t*)mesh_host_alloc(sz_f, &pf);
      if (c->mesh_keys) out->edge_keys = (int64_t*)mesh_host_alloc(sz_k, &pk);
      if (out->vertices && out->faces && (!c->mesh_keys || out->edge_keys) && pinned && pf && pk) {
        host.direct = true;
        chain.verts = out->vertices;
        chain.keys = c->mesh_keys ? (long long*)out->edge_keys : nullptr;
        chain.faces = (int*)out->faces;
        return VCY_OK;
      }
      host.release_mesh();
    }
    VCY_HIP_CHECK(c->d_mc_out.grow(sz_v + sz_k + sz_f, s));
    chain.verts = (float*)c->d_mc_out;
    chain.keys = c->mesh_keys ? (long long*)((char*)c->d_mc_out + sz_v) : nullptr;
    chain.faces = (int*)((char*)c->d_mc_out + sz_v + sz_k);
    return VCY_OK;
  }

  // Normals (vcy_extract_iso_normals): two more launches behind mc_emit, behind the same capacity checks (they read
  // the counts themselves), enqueued again with the chain when a guess was too small.  Their own event pair:
  // last_extract_device_ms stays "the mesh kernels".
  int enqueue_normals() {
    const size_t sz_vn =
        (which & VCY_NORMALS_VERTEX) ? align256(sizeof(float) * 3 * (size_t)std::max<int64_t>(chain.cap_verts, 1)) : 0;
    const size_t sz_fn =
        (which & VCY_NORMALS_FACE) ? align256(sizeof(float) * 3 * (size_t)std::max<int64_t>(chain.cap_faces, 1)) : 0;
    VCY_HIP_CHECK(c->d_mc_normals.grow(sz_vn + sz_fn, s));
    d_vn = sz_vn ? (float*)c->d_mc_normals : nullptr;
    d_fn = sz_fn ? (float*)((char*)c->d_mc_normals + sz_vn) : nullptr;
    VCY_HIP_CHECK(c->ev_nrm_begin.ensure());
    VCY_HIP_CHECK(c->ev_nrm_end.ensure());
    NormalsLaunch a;
    a.T = chain.T;
    a.act = chain.act;
    a.cell_list = chain.cell_list;
    a.ncells_dev = chain.ncells_dev;
    a.cap_cells = chain.cap_cells;
    a.info = chain.info;
    a.block_offs = chain.block_offs;
    a.grand_total_dev = chain.grand_total_dev;
    a.cap_verts = chain.cap_verts;
    a.cap_faces = chain.cap_faces;
    a.verts = chain.verts;
    a.faces = chain.faces;
    a.vertex_normals = d_vn;
    a.face_normals = d_fn;
    // a z-slab (vcy_extract_iso_normals_slab): the seam vertices are left to the host, the layer counts it needs come
    // back in the report block, behind the four words of mc_emit
    a.slab = (c->z0 != 0 || c->z1 != c->nz || c->halo_lo != 0) ? 1 : 0;
    a.open_top = c->z1 < c->nz ? 1 : 0;
    a.word_cell_off = chain.word_cell_off;
    a.block_cell_offs = chain.block_cells;
    a.ghost_cells_dev = chain.block_cells + p.G / kWordsPerBlock;
    a.report = layer_faces ? (u64*)c->h_mc_report + 4 : nullptr;
    VCY_HIP_CHECK(hipEventRecord(c->ev_nrm_begin, s));
    VCY_HIP_CHECK(launch_normals(s, p, a));
    VCY_HIP_CHECK(hipEventRecord(c->ev_nrm_end, s));
    normals_timed = true;
    return VCY_OK;
  }

  // The chain behind the cell search: owners, emit, the end of the mesh kernels' timer, then the normals.  With guessed
  // capacities nothing is read back in between; with cap_v == kFromTotals the output arrays are sized (with the same
  // headroom as the guesses, so that the next extraction does not reallocate) from the totals of the owner pass.
  int run_chain(int64_t cap_cells, int64_t cap_v, int64_t cap_f) {
    int rc = cell_buffers(cap_cells);
    if (rc == VCY_OK) rc = launch_owners(s, p, chain, scan_slot(1));
    if (rc != VCY_OK) return rc;
    if (cap_v == kFromTotals) {
      VCY_HIP_CHECK(hipMemcpyAsync((void*)&report[2], chain.grand_total_dev, sizeof(u64), hipMemcpyDeviceToHost, s));
      VCY_HIP_CHECK(hipStreamSynchronize(s));
      nv = (int64_t)(report[2] >> 32);
      nf = (int64_t)(report[2] & 0xFFFFFFFFull);
      cap_v = with_headroom(nv), cap_f = with_headroom(nf);
    }
    rc = output_buffers(cap_v, cap_f);
    if (rc == VCY_OK) rc = launch_emit(s, p, chain);
    if (rc != VCY_OK) return rc;
    // (the end of the kernels: last_extract_device_ms is "kernels only")
    VCY_HIP_CHECK(hipEventRecord(c->ev_mc_end, s));
    end_recorded = true;
    return wants_normals() ? enqueue_normals() : VCY_OK;
  }

  // first extraction of a context, or a guess that was too small: the numbers of cells, read back before anything is sized
  int fetch_counts() {
    VCY_HIP_CHECK(hipMemcpyAsync((void*)&report[0], chain.ncells_dev, sizeof(u64), hipMemcpyDeviceToHost, s));
    VCY_HIP_CHECK(hipMemcpyAsync((void*)&report[1], chain.block_cells + p.G / kWordsPerBlock, sizeof(u64),
                                 hipMemcpyDeviceToHost, s));
    VCY_HIP_CHECK(hipStreamSynchronize(s));
    ncells = (int64_t)report[0];
    nv = nf = nforeign = 0;
    if (ncells > 0xFFFFFFFFLL) {
      set_error("too many surface cells");
      return VCY_ERR_TOO_MANY_VOXELS;
    }
    return VCY_OK;
  }

  // what mc_emit (and the normals' layer count) left in the report block; valid after a wait for the stream
  void read_report() {
    ncells = (int64_t)report[0];
    nv = (int64_t)(report[2] >> 32);
    nf = (int64_t)(report[2] & 0xFFFFFFFFull);
    nforeign = (int64_t)report[3];
    first_layer_faces = (int64_t)report[4];  // (written by the normals' layer count, when asked for)
    last_layer_faces = (int64_t)report[5];
  }

  // (on failure the guard releases both structs)
  int copy_normals(float** dst, const float* src, int64_t n) {
    *dst = (float*)mesh_host_alloc(sizeof(float) * 3 * (size_t)n);
    if (!*dst) {
      set_error("out of host memory for the normals");
      return VCY_ERR_INTERNAL;
    }
    VCY_HIP_CHECK(hipMemcpyAsync(*dst, src, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToHost, s));
    return VCY_OK;
  }

  // The mesh into *out: already there (direct), or page-locked host buffers and three DMAs in flight on the stream.
  int deliver() {
    const bool was_direct = host.direct;
    if (host.direct && ncells > 0 && (nv > 0 || nf > 0)) {
      // the arrays are already where the caller reads them; an empty side has no array
      if (nv == 0) {
        mesh_host_free(out->vertices);
        mesh_host_free(out->edge_keys);
        out->vertices = nullptr, out->edge_keys = nullptr;
      }
      if (nf == 0) {
        mesh_host_free(out->faces);
        out->faces = nullptr;
      }
    } else {
      if (host.direct) host.release_mesh();  // (an empty mesh)
      if (nv > 0) {
        out->vertices = (float*)mesh_host_alloc(sizeof(float) * 3 * (size_t)nv);
        if (c->mesh_keys) out->edge_keys = (int64_t*)mesh_host_alloc(sizeof(int64_t) * 2 * (size_t)nv);
      }
      if (nf > 0) out->faces = (int32_t*)mesh_host_alloc(sizeof(int32_t) * 3 * (size_t)nf);
      if ((nv > 0 && (!out->vertices || (c->mesh_keys && !out->edge_keys))) || (nf > 0 && !out->faces)) {
        set_error("out of host memory for the mesh");
        return VCY_ERR_INTERNAL;
      }
      if (nv > 0) {
        VCY_HIP_CHECK(hipMemcpyAsync(out->vertices, chain.verts, sizeof(float) * 3 * (size_t)nv, hipMemcpyDeviceToHost, s));
        if (c->mesh_keys)
          VCY_HIP_CHECK(hipMemcpyAsync(out->edge_keys, chain.keys, sizeof(long long) * 2 * (size_t)nv, hipMemcpyDeviceToHost, s));
      }
      if (nf > 0) VCY_HIP_CHECK(hipMemcpyAsync(out->faces, chain.faces, sizeof(int) * 3 * (size_t)nf, hipMemcpyDeviceToHost, s));
      int rc = VCY_OK;
      if ((which & VCY_NORMALS_VERTEX) && ncells > 0 && nv > 0) rc = copy_normals(&normals_out->vertex_normals, d_vn, nv);
      if (rc == VCY_OK && (which & VCY_NORMALS_FACE) && ncells > 0 && nf > 0) rc = copy_normals(&normals_out->face_normals, d_fn, nf);
      if (rc != VCY_OK) return rc;
      if (nv > 0 || nf > 0) VCY_HIP_CHECK(hipStreamSynchronize(s));
      if (normals_timed && ncells > 0) VCY_HIP_CHECK(hipEventSynchronize(c->ev_nrm_end));
      if (normals_timed && ncells > 0) VCY_HIP_CHECK(hipEventElapsedTime(&c->last_normals_device_ms, c->ev_nrm_begin, c->ev_nrm_end));
    }
    out->n_vertices = nv;
    out->n_faces = nf;
    if (layer_faces && ncells > 0 && nf > 0) layer_faces[0] = first_layer_faces, layer_faces[1] = last_layer_faces;
    if (timing) {
      t_ph[4] = now_us();
      fprintf(stderr, "[vcy mc timing] setup %.1f us | enqueue %.1f | wait %.1f | events %.1f | mesh to host %.1f | total %.1f "
                      "(direct %d, %lld cells, %lld v, %lld f, kernels %.1f us)\n",
              t_ph[0] - t_begin, t_ph[1] - t_ph[0], t_ph[2] - t_ph[1], t_ph[3] - t_ph[2], t_ph[4] - t_ph[3], t_ph[4] - t_begin,
              was_direct ? 1 : 0, (long long)ncells, (long long)nv, (long long)nf, c->last_extract_device_ms * 1e3);
    }
    return VCY_OK;
  }

  int run(double iso, int linear_interp) {
    bool any_cells = false;
    int rc = plan(iso, linear_interp, &any_cells);
    if (rc != VCY_OK || !any_cells) return rc;
    if ((rc = scratch()) != VCY_OK) return rc;
    if ((rc = find_cells()) != VCY_OK) return rc;
    timing = c->mc_timing != 0;
    if (timing) t_begin = t_ph[0] = now_us();
    bool done = false;
    if (c->mc_hint_cells > 0) {
      const int64_t cap_cells = with_headroom(c->mc_hint_cells);
      const int64_t cap_v = with_headroom(c->mc_hint_verts), cap_f = with_headroom(c->mc_hint_faces);
      if ((rc = run_chain(cap_cells, cap_v, cap_f)) != VCY_OK) return rc;
      if (timing) t_ph[1] = now_us();
      VCY_HIP_CHECK(hipStreamSynchronize(s));  // the ONE wait of an extraction whose mesh went straight to host memory
      if (timing) t_ph[2] = now_us();
      read_report();
      done = ncells <= cap_cells && nv <= cap_v && nf <= cap_f;
      if (ncells == 0) nv = nf = 0;
      if (!done) host.release_mesh();
    }
    if (!done) {
      if ((rc = fetch_counts()) != VCY_OK) return rc;
      if (ncells > 0) {
        if ((rc = run_chain(with_headroom(ncells), kFromTotals, kFromTotals)) != VCY_OK) return rc;
        VCY_HIP_CHECK(hipStreamSynchronize(s));
        read_report();
      } else {
        end_recorded = false;
      }
    }
    if (ncells > 0) out->n_foreign_vertices = nforeign;
    c->mc_hint_cells = ncells;
    c->mc_hint_verts = nv;
    c->mc_hint_faces = nf;
    if (!end_recorded) VCY_HIP_CHECK(hipEventRecord(c->ev_mc_end, s));
    VCY_HIP_CHECK(hipEventSynchronize(c->ev_mc_end));
    VCY_HIP_CHECK(hipEventElapsedTime(&c->last_extract_device_ms, c->ev_mc_begin, c->ev_mc_end));
    if (timing) t_ph[3] = now_us();
    if (staged) {  // (the counts of the one wait above; an empty mesh has no arrays)
      const bool any = ncells > 0 && nv > 0 && nf > 0;
      *staged = StagedMesh{any ? chain.verts : nullptr, any ? chain.faces : nullptr, any ? nv : 0, any ? nf : 0, p,
                           CornerRowsLaunch{chain.T, chain.act, chain.cell_list, ncells, nv, nf, chain.info, chain.block_offs,
                                            chain.word_cell_off, chain.block_cells, nullptr, nullptr, nullptr, nullptr}};
      return VCY_OK;
    }
    return deliver();
  }
};

}  // namespace

int extract_iso(vcy_ctx* c, double iso, int linear_interp, vcy_mesh* out, int which, vcy_mesh_normals* normals_out,
                int64_t* layer_faces) {
  out->n_vertices = out->n_faces = out->n_foreign_vertices = 0;
  out->vertices = nullptr;  // an empty mesh has no arrays
  out->faces = nullptr;
  out->edge_keys = nullptr;
  if (c->halo_lo && !c->st.halo_valid) {
    set_error("halo slices not installed: call vcy_halo_pack / all-gather / vcy_halo_unpack first");
    return VCY_ERR_NOT_INITIALIZED;
  }
  Extraction x(c, out, which, normals_out, layer_faces);
  const int rc = x.run(iso, linear_interp);
  if (rc == VCY_OK) x.host.armed = false;
  return rc;
}

// The extraction of extract_iso with the mesh left where mc_emit wrote it, the device staging vcy_ctx::d_mc_out, whatever
// "mcdirect" says: the extraction chain's first stage (mesh_chain.hip).  The counts are those of the extraction's own wait.
int extract_iso_staged(vcy_ctx* c, double iso, int linear_interp, StagedMesh* staged) {
  *staged = StagedMesh{};
  vcy_mesh none{};
  Extraction x(c, &none, 0, nullptr, nullptr);
  x.staged = staged;
  return x.run(iso, linear_interp);
}

}  // namespace vcy
