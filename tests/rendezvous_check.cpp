// Stand-alone check of vcy_rendezvous_exchange (vacancy_amd/csrc/rendezvous.hip) for a host sanitizer build: no GPU, no
// HIP runtime, its own vcy::set_error.  `make -C vacancy_amd/csrc rendezvous_check` builds it from rendezvous.hip alone
// with AddressSanitizer and UBSan on the host side and runs it (CPU only).
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <unistd.h>

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

int main() {
  char dir[] = "/tmp/vcy_rendezvous_XXXXXX";
  CHECK(mkdtemp(dir) != nullptr);
  const std::string base(dir);

  // four ranks as four threads: rank 0's 128 bytes arrive at every rank (the late ones poll for the file)
  const int world = 4;
  const std::string where = "file:" + base + "/id";
  std::vector<std::vector<unsigned char>> payload((size_t)world, std::vector<unsigned char>(128, 0));
  for (int i = 0; i < 128; ++i) payload[0][(size_t)i] = (unsigned char)((i * 7 + 3) & 255);
  std::vector<int> rc((size_t)world, -1);
  std::vector<std::thread> threads;
  for (int r = world - 1; r >= 0; --r)
    threads.emplace_back([&, r] { rc[(size_t)r] = vcy_rendezvous_exchange(r, world, where.c_str(), payload[(size_t)r].data(), 20000); });
  for (std::thread& t : threads) t.join();
  for (int r = 0; r < world; ++r) {
    CHECK(rc[(size_t)r] == VCY_OK);
    CHECK(payload[(size_t)r] == payload[0]);
  }

  // rank 0 absent: the others give up after their timeout and say what did not appear
  std::vector<unsigned char> buf(128, 0);
  const std::string never = "file:" + base + "/never";
  CHECK(vcy_rendezvous_exchange(1, 2, never.c_str(), buf.data(), 50) == VCY_ERR_INTERNAL);
  CHECK(std::strstr(vcy::g_error, "did not appear") != nullptr);

  // malformed targets and arguments are refused
  CHECK(vcy_rendezvous_exchange(1, 2, "smoke:signals", buf.data(), 50) == VCY_ERR_INVALID_ARG);
  CHECK(std::strstr(vcy::g_error, "file:<path>") != nullptr);
  CHECK(vcy_rendezvous_exchange(1, 2, "file:", buf.data(), 50) == VCY_ERR_INVALID_ARG);
  CHECK(vcy_rendezvous_exchange(1, 2, "tcp:host:notaport", buf.data(), 50) == VCY_ERR_INVALID_ARG);
  CHECK(vcy_rendezvous_exchange(0, 2, nullptr, buf.data(), 50) == VCY_ERR_INVALID_ARG);
  CHECK(vcy_rendezvous_exchange(2, 2, where.c_str(), buf.data(), 50) == VCY_ERR_INVALID_ARG);
  CHECK(vcy_rendezvous_exchange(0, 1, "file:/nowhere", buf.data(), 50) == VCY_OK);  // one rank: nothing to exchange

  (void)::unlink((base + "/id").c_str());
  (void)::rmdir(dir);
  std::puts("rendezvous_check: ok");
  return 0;
}
