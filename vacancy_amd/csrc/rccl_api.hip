// The dlopen'd RCCL table and the record of the last collective (rccl_api.h).
#include <dlfcn.h>

#include <cstdio>

#include "rccl_api.h"

namespace vcy {

std::mutex g_rccl_mutex;
RcclApi g_rccl;

namespace {

struct LastCollective {
  int ranks = 0;
  int64_t bytes_per_rank = 0;
  int64_t calls = 0;
  int version = 0;
} g_last;
thread_local std::string g_last_text;

}  // namespace

bool load_rccl() {
  if (g_rccl.handle) return true;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  void* h = nullptr;
  for (const char* n : names) {
    h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (h) {
      g_rccl.path = n;
      break;
    }
  }
  if (!h) {
    set_error("vcy_halo_allgather: librccl.so not found (%s)", dlerror());
    return false;
  }
#define VCY_SYM(field, name)                                              \
  do {                                                                    \
    *(void**)(&g_rccl.field) = dlsym(h, name);                            \
    if (!g_rccl.field) {                                                  \
      set_error("vcy_halo_allgather: %s missing from librccl.so", name);  \
      dlclose(h);                                                         \
      return false;                                                       \
    }                                                                     \
  } while (0)
  VCY_SYM(GetVersion, "ncclGetVersion");
  VCY_SYM(CommInitAll, "ncclCommInitAll");
  VCY_SYM(GetUniqueId, "ncclGetUniqueId");
  VCY_SYM(CommInitRank, "ncclCommInitRank");
  VCY_SYM(CommDestroy, "ncclCommDestroy");
  VCY_SYM(AllGather, "ncclAllGather");
  VCY_SYM(GroupStart, "ncclGroupStart");
  VCY_SYM(GroupEnd, "ncclGroupEnd");
  VCY_SYM(GetErrorString, "ncclGetErrorString");
#undef VCY_SYM
  *(void**)(&g_rccl.CommAbort) = dlsym(h, "ncclCommAbort");
  g_rccl.handle = h;
  return true;
}

void note_collective(int ranks, size_t bytes_per_rank) {
  g_last.ranks = ranks;
  g_last.bytes_per_rank = (int64_t)bytes_per_rank;
  g_last.calls += 1;
  (void)g_rccl.GetVersion(&g_last.version);
}

}  // namespace vcy

using namespace vcy;

extern "C" const char* vcy_last_collective(void) {
  std::lock_guard<std::mutex> lock(g_rccl_mutex);
  char buf[256];
  if (g_last.calls == 0) {
    g_last_text = "none";
  } else {
    snprintf(buf, sizeof(buf), "backend=rccl op=ncclAllGather version=%d ranks=%d bytes_per_rank=%lld calls=%lld lib=%s",
             g_last.version, g_last.ranks, (long long)g_last.bytes_per_rank, (long long)g_last.calls,
             g_rccl.path.c_str());
    g_last_text = buf;
  }
  return g_last_text.c_str();
}
