// RCCL as the library uses it: the table of entry points of a librccl.so opened on first use (dlopen: the carve path
// needs no collective, and a host process that already carries an RCCL -- PyTorch ships its own librccl.so -- keeps
// using that one), the owner of one communicator, the communicator groups cached per device list, and the record behind
// vcy_last_collective.  Included by rccl_api.hip and its two users, halo_exchange.hip and carve_stream.hip; nothing
// else sees <rccl/rccl.h>.
#pragma once

#include <rccl/rccl.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "vcy_internal.h"

namespace vcy {

struct RcclApi {
  void* handle = nullptr;
  ncclResult_t (*GetVersion)(int*) = nullptr;
  ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;                        // (process-per-GPU form, vcy_comm_create)
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;  // (optional: the error path of the sharded producer)
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string path;
};

// One lock for everything that goes through the table: the caches of communicators and producers, the collectives.
extern std::mutex g_rccl_mutex;
extern RcclApi g_rccl;

bool load_rccl();  // (g_rccl_mutex held) false, with the error set, when librccl.so or one of its symbols is missing

#define VCY_NCCL_CHECK(expr)                                                                  \
  do {                                                                                        \
    ncclResult_t _r = (expr);                                                                 \
    if (_r != ncclSuccess) {                                                                  \
      set_error("%s failed: %s (%s:%d)", #expr, g_rccl.GetErrorString(_r), __FILE__, __LINE__); \
      return VCY_ERR_HIP;                                                                     \
    }                                                                                         \
  } while (0)

// What vcy_last_collective reports: called (g_rccl_mutex held) by every halo all-gather that completed.
void note_collective(int ranks, size_t bytes_per_rank);

// One communicator: move-only, empty by default, destroyed (ncclCommDestroy) with its holder.
struct CommDestroyer { void operator()(ncclComm_t c) const { (void)g_rccl.CommDestroy(c); } };
struct Comm : std::unique_ptr<std::remove_pointer<ncclComm_t>::type, CommDestroyer> {
  using unique_ptr::unique_ptr;
  // ncclCommAbort, where the loaded library has it: an aborted communicator is gone, the holder is empty afterwards.
  void abort() {
    if (*this && g_rccl.CommAbort) (void)g_rccl.CommAbort(release());
  }
};

// The collective stream of one device and the two buffers a halo all-gather runs between.  The stream is declared first,
// so it goes last; the destructor's body waits for it, on its device, before the members go.
struct HaloStaging {
  int device = 0;
  Stream stream;
  DeviceBuf<char> send, recv;

  ~HaloStaging() {
    if (!stream) return;
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(stream);
  }
  // Grow-only; what is in flight on the staging's stream is waited for before a buffer is replaced.
  int reserve(size_t send_bytes, size_t recv_bytes) {
    VCY_HIP_CHECK(hipSetDevice(device));
    VCY_HIP_CHECK(send.grow(send_bytes, stream));
    VCY_HIP_CHECK(recv.grow(recv_bytes, stream));
    return VCY_OK;
  }
};

// Communicators and staging buffers are cached per device list (creating a communicator costs
// hundreds of milliseconds; an extraction per carved view would pay it every time).
struct HaloGroup {
  std::vector<int> devices;
  std::vector<Comm> comms;           // per device; declared before the staging: destroyed after every device's buffers
  std::vector<HaloStaging> staging;  // per device
  explicit HaloGroup(const std::vector<int>& d) : devices(d), comms(d.size()), staging(d.size()) {}
};
int get_group(const std::vector<int>& devices, HaloGroup** out);  // the cached group of a device list (halo_exchange.hip); g_rccl_mutex held
void drop_group(HaloGroup* g);  // out of the cache and destroyed (after its communicators were aborted)
// The caches of owners keyed by device list (here and in carve_stream.hip): the cached owner of `devices` or null, and
// an owner out of its cache and destroyed.
template <class G>
G* find_in(const std::vector<std::unique_ptr<G>>& cache, const std::vector<int>& devices) {
  for (const std::unique_ptr<G>& g : cache)
    if (g->devices == devices) return g.get();
  return nullptr;
}
template <class G>
void drop_from(std::vector<std::unique_ptr<G>>& cache, const G* g) {
  cache.erase(std::remove_if(cache.begin(), cache.end(), [g](const std::unique_ptr<G>& p) { return p.get() == g; }), cache.end());
}
void drop_producers();          // the cached producer groups of carve_stream.hip (vcy_halo_shutdown)

}  // namespace vcy
