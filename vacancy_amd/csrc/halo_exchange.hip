// Halo exchange of a z-slab sharded grid: a single RCCL all-gather.
//
// Marching-cubes cells span z-1..z (reference src/vacancy/marching_cubes.cc:93-101), so before
// extraction every slab needs the last two xy-slices of the slab below it.  The north star asks for
// "a single RCCL all-gather of boundary slabs": every device contributes the packs (vcy_halo_pack
// layout) of the slabs it holds, ncclAllGather hands every device every pack, and each slab installs
// the pack of the slab that ends at its z_begin.  Two forms: inside ONE process that drives all GPUs of the node
// (vcy_halo_allgather: one communicator rank per distinct DEVICE, ncclCommInitAll; several slabs of one device share
// that device's rank), and one process per GPU without torch (vcy_comm_create + vcy_halo_allgather_ranks, below).  The
// torch form of the latter is vacancy_amd/dist.py (torch.distributed all_gather_into_tensor, which is RCCL as well).
#include <algorithm>
#include <cstring>

#include "rccl_api.h"

namespace vcy {

namespace {
// On the heap and never destroyed: what is still cached when the process ends is left alone, as raw pointers were (no
// GPU or RCCL call runs from a static destructor); vcy_halo_shutdown is the only release.
auto& g_groups = *new std::vector<std::unique_ptr<HaloGroup>>;
}  // namespace

int get_group(const std::vector<int>& devices, HaloGroup** out) {
  if ((*out = find_in(g_groups, devices))) return VCY_OK;
  std::unique_ptr<HaloGroup> g(new HaloGroup(devices));
  const int nd = (int)devices.size();
  std::vector<ncclComm_t> raw((size_t)nd, nullptr);
  ncclResult_t r = g_rccl.CommInitAll(raw.data(), nd, devices.data());
  if (r != ncclSuccess) {
    set_error("ncclCommInitAll(%d devices) failed: %s", nd, g_rccl.GetErrorString(r));
    return VCY_ERR_HIP;
  }
  for (int d = 0; d < nd; ++d) g->comms[(size_t)d] = Comm(raw[(size_t)d]);
  for (int d = 0; d < nd; ++d) {
    hipError_t e = hipSetDevice(devices[(size_t)d]);
    g->staging[(size_t)d].device = devices[(size_t)d];
    if (e == hipSuccess) e = g->staging[(size_t)d].stream.create(hipStreamNonBlocking);
    if (e != hipSuccess) {  // nothing half-built stays behind (a retry would initialise the communicators again)
      set_error("vcy_halo_allgather: stream on device %d: %s", devices[(size_t)d], hipGetErrorString(e));
      return VCY_ERR_HIP;
    }
  }
  *out = g.get();
  g_groups.push_back(std::move(g));
  return VCY_OK;
}

void drop_group(HaloGroup* g) { drop_from(g_groups, g); }

}  // namespace vcy

using namespace vcy;

extern "C" {

int vcy_halo_allgather(vcy_ctx* const* slabs, int n_slabs) {
  if (!slabs || n_slabs <= 0) {
    set_error("vcy_halo_allgather: no slabs");
    return VCY_ERR_INVALID_ARG;
  }
  // the slabs must tile z in order: slab i ends where slab i + 1 begins, same xy grid and counter width
  for (int i = 0; i < n_slabs; ++i) {
    const vcy_ctx* c = slabs[i];
    if (!c) return VCY_ERR_INVALID_ARG;
    if (i > 0) {
      const vcy_ctx* p = slabs[i - 1];
      if (p->z1 != c->z0 || p->nx != c->nx || p->ny != c->ny || p->cnt_bytes_wire != c->cnt_bytes_wire) {
        set_error("vcy_halo_allgather: slab %d does not continue slab %d", i, i - 1);
        return VCY_ERR_INVALID_ARG;
      }
    }
    if (n_slabs > 1 && c->nz_local() < 2) {
      set_error("a slab needs at least 2 slices to exchange halos");
      return VCY_ERR_INVALID_ARG;
    }
  }
  if (slabs[0]->z0 != 0) {
    set_error("vcy_halo_allgather: the first slab must start at z = 0");
    return VCY_ERR_INVALID_ARG;
  }
  if (n_slabs == 1) {
    slabs[0]->st.halo_installed();  // a whole grid: nothing below
    return VCY_OK;
  }
  std::lock_guard<std::mutex> lock(g_rccl_mutex);
  if (!load_rccl()) return VCY_ERR_UNSUPPORTED;

  // one communicator rank per distinct device, in order of first appearance
  std::vector<int> devices;
  std::vector<int> rank_of((size_t)n_slabs), slot_of((size_t)n_slabs);
  std::vector<int> held;  // slabs per rank
  for (int i = 0; i < n_slabs; ++i) {
    const int dev = slabs[i]->device;
    size_t r = 0;
    while (r < devices.size() && devices[r] != dev) ++r;
    if (r == devices.size()) {
      devices.push_back(dev);
      held.push_back(0);
    }
    rank_of[(size_t)i] = (int)r;
    slot_of[(size_t)i] = held[r]++;
  }
  const int nd = (int)devices.size();
  const int kmax = *std::max_element(held.begin(), held.end());  // equal send counts: pad to the most slabs a rank holds
  const size_t pack = (size_t)vcy_halo_bytes(slabs[0]);
  const size_t send_bytes = pack * (size_t)kmax, recv_bytes = send_bytes * (size_t)nd;
  HaloGroup* g = nullptr;
  int rc = get_group(devices, &g);
  if (rc != VCY_OK) return rc;
  for (HaloStaging& st : g->staging) {
    rc = st.reserve(send_bytes, recv_bytes);
    if (rc != VCY_OK) return rc;
  }

  // pack: every slab's last two slices into its rank's send buffer (applies queued views first)
  for (int i = 0; i < n_slabs; ++i) {
    rc = vcy_halo_pack(slabs[i], g->staging[(size_t)rank_of[(size_t)i]].send + pack * (size_t)slot_of[(size_t)i]);
    if (rc != VCY_OK) return rc;
  }
  for (int i = 0; i < n_slabs; ++i) {
    VCY_HIP_CHECK(hipSetDevice(slabs[i]->device));
    VCY_HIP_CHECK(hipStreamSynchronize(slabs[i]->stream));
  }
  // the single collective of the path
  VCY_NCCL_CHECK(g_rccl.GroupStart());
  for (int d = 0; d < nd; ++d) {
    HaloStaging& st = g->staging[(size_t)d];
    ncclResult_t r = g_rccl.AllGather(st.send, st.recv, send_bytes, ncclUint8, g->comms[(size_t)d].get(), st.stream);
    if (r != ncclSuccess) {
      (void)g_rccl.GroupEnd();
      set_error("ncclAllGather failed: %s", g_rccl.GetErrorString(r));
      return VCY_ERR_HIP;
    }
  }
  VCY_NCCL_CHECK(g_rccl.GroupEnd());
  for (int d = 0; d < nd; ++d) {
    VCY_HIP_CHECK(hipSetDevice(devices[(size_t)d]));
    VCY_HIP_CHECK(hipStreamSynchronize(g->staging[(size_t)d].stream));
  }
  // install: slab i takes the pack of slab i - 1 out of its own device's gathered buffer
  for (int i = 0; i < n_slabs; ++i) {
    const char* src = nullptr;
    if (i > 0)
      src = g->staging[(size_t)rank_of[(size_t)i]].recv + send_bytes * (size_t)rank_of[(size_t)i - 1] +
            pack * (size_t)slot_of[(size_t)i - 1];
    rc = vcy_halo_install(slabs[i], src);
    if (rc != VCY_OK) return rc;
  }
  for (int i = 0; i < n_slabs; ++i) {  // the staging is reused by the next exchange
    VCY_HIP_CHECK(hipSetDevice(slabs[i]->device));
    VCY_HIP_CHECK(hipStreamSynchronize(slabs[i]->stream));
  }
  note_collective(nd, send_bytes);
  return VCY_OK;
}

void vcy_halo_shutdown(void) {
  std::lock_guard<std::mutex> lock(g_rccl_mutex);
  drop_producers();
  g_groups.clear();
}

}  // extern "C"

/* ---- one process per GPU, without torch ---------------------------------------------------------------------------
 * The north star keeps the host in C++; its multi-GPU form is "one process per GPU ... a single RCCL all-gather of
 * boundary slabs".  vacancy_amd/dist.py does that exchange through torch.distributed; a C++ host has no torch.  Here
 * is the same exchange for it: every process creates a vcy_comm (rank r of `world`, its device), the ncclUniqueId of
 * rank 0 reaches the others through a RENDEZVOUS that needs nothing but the filesystem or a TCP port of the node
 * ("file:<path>" or "tcp:<host>:<port>", rendezvous.hip), ncclCommInitRank builds the communicator, and
 * vcy_halo_allgather_ranks is the one collective: this rank's slabs (slab ids rank, rank + world, ...) pack their last
 * two slices, ONE ncclAllGather hands every rank every pack (rank-major, as vacancy_amd.dist.exchange_halo lays them
 * out), every slab installs the pack of the slab below it.  No reference counterpart (the reference is single-process
 * OpenMP).                                                                                                            */
static_assert(sizeof(ncclUniqueId) == 128, "rendezvous payload = one ncclUniqueId");

struct vcy_comm {
  int rank = 0, world = 1;
  Comm comm;        // declared before the staging: destroyed after its buffers
  HaloStaging st;
};

extern "C" {

int vcy_comm_create(int rank, int world, int device_id, const char* where, int timeout_ms, vcy_comm** out) {
  if (!out || rank < 0 || world < 1 || rank >= world) {
    set_error("vcy_comm_create: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  *out = nullptr;
  std::lock_guard<std::mutex> lock(g_rccl_mutex);
  if (!load_rccl()) return VCY_ERR_UNSUPPORTED;
  VCY_HIP_CHECK(hipSetDevice(device_id));
  ncclUniqueId id;
  std::memset(&id, 0, sizeof(id));
  if (rank == 0) VCY_NCCL_CHECK(g_rccl.GetUniqueId(&id));
  {
    const int rc = vcy_rendezvous_exchange(rank, world, where ? where : "", &id, timeout_ms > 0 ? timeout_ms : 120000);
    if (rc != VCY_OK && world > 1) return rc;
  }
  std::unique_ptr<vcy_comm> c(new vcy_comm());
  c->rank = rank, c->world = world, c->st.device = device_id;
  ncclComm_t raw = nullptr;
  const ncclResult_t r = g_rccl.CommInitRank(&raw, world, id, rank);
  if (r != ncclSuccess) {
    set_error("ncclCommInitRank(rank %d of %d, device %d) failed: %s", rank, world, device_id, g_rccl.GetErrorString(r));
    return VCY_ERR_HIP;
  }
  c->comm = Comm(raw);
  if (c->st.stream.create(hipStreamNonBlocking) != hipSuccess) {
    set_error("vcy_comm_create: stream");
    return VCY_ERR_HIP;
  }
  *out = c.release();
  return VCY_OK;
}

void vcy_comm_destroy(vcy_comm* c) {
  if (!c) return;
  std::lock_guard<std::mutex> lock(g_rccl_mutex);
  delete c;
}

int vcy_halo_allgather_ranks(vcy_comm* cm, vcy_ctx* const* my_slabs, int n_my_slabs) {
  if (!cm || !my_slabs || n_my_slabs <= 0) {
    set_error("vcy_halo_allgather_ranks: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  for (int i = 0; i < n_my_slabs; ++i)
    if (!my_slabs[i] || my_slabs[i]->device != cm->st.device) {
      set_error("vcy_halo_allgather_ranks: slab %d is not a context on this rank's device", i);
      return VCY_ERR_INVALID_ARG;
    }
  const int k = n_my_slabs, world = cm->world;
  if (world * k == 1) {
    my_slabs[0]->st.halo_installed();
    return VCY_OK;
  }
  std::lock_guard<std::mutex> lock(g_rccl_mutex);
  const size_t pack = (size_t)vcy_halo_bytes(my_slabs[0]);
  const size_t send_bytes = pack * (size_t)k, recv_bytes = send_bytes * (size_t)world;
  {
    const int rc = cm->st.reserve(send_bytes, recv_bytes);  // (sets the rank's device current)
    if (rc != VCY_OK) return rc;
  }
  for (int i = 0; i < k; ++i) {
    const int rc = vcy_halo_pack(my_slabs[i], cm->st.send + pack * (size_t)i);  // (applies queued views first)
    if (rc != VCY_OK) return rc;
  }
  for (int i = 0; i < k; ++i) VCY_HIP_CHECK(hipStreamSynchronize(my_slabs[i]->stream));
  // the single collective of the path
  VCY_NCCL_CHECK(g_rccl.AllGather(cm->st.send, cm->st.recv, send_bytes, ncclUint8, cm->comm.get(), cm->st.stream));
  VCY_HIP_CHECK(hipStreamSynchronize(cm->st.stream));
  for (int i = 0; i < k; ++i) {
    const int sid = cm->rank + i * world;  // this slab's id; the slab below it is sid - 1, held by rank (sid - 1) % world
    const char* src = nullptr;
    if (sid > 0) {
      const int below = sid - 1;
      src = cm->st.recv + ((size_t)(below % world) * (size_t)k + (size_t)(below / world)) * pack;
    }
    const int rc = vcy_halo_install(my_slabs[i], src);
    if (rc != VCY_OK) return rc;
  }
  for (int i = 0; i < k; ++i) VCY_HIP_CHECK(hipStreamSynchronize(my_slabs[i]->stream));
  note_collective(world, send_bytes);
  return VCY_OK;
}

}  // extern "C"
