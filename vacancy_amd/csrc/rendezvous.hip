// The rendezvous of a job that runs one process per GPU without torch: 128 bytes of rank 0 (the ncclUniqueId of
// vcy_comm_create, halo_exchange.hip) reach every other rank through nothing but the filesystem or a TCP port of the
// node ("file:<path>" or "tcp:<host>:<port>").  Host code only -- no GPU, nothing of the HIP runtime or of RCCL --, so it
// links into a program without any device part.
#include <arpa/inet.h>
#include <fcntl.h>
#include <netdb.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <sys/socket.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <string>

#include "vacancy_hip.h"

namespace vcy {
void set_error(const char* fmt, ...);

namespace {

constexpr size_t kRendezvousBytes = 128;  // sizeof(ncclUniqueId), asserted where the id is made (halo_exchange.hip)

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

bool write_all(int fd, const void* buf, size_t n) {
  const char* p = (const char*)buf;
  while (n > 0) {
    const ssize_t w = ::write(fd, p, n);
    if (w <= 0) return false;
    p += w;
    n -= (size_t)w;
  }
  return true;
}
bool read_all(int fd, void* buf, size_t n) {
  char* p = (char*)buf;
  while (n > 0) {
    const ssize_t r = ::read(fd, p, n);
    if (r <= 0) return false;
    p += r;
    n -= (size_t)r;
  }
  return true;
}

// file:<path> -- rank 0 writes <path>.tmp and renames it to <path> (atomic: a reader sees all 128 bytes or no file);
// the others poll for it.  Rank 0 removes a stale file of an earlier job before it writes; the path must be private to
// the job (bench-style: include the job's port or pid).
int rendezvous_file(const std::string& path, int rank, void* payload, int timeout_ms) {
  if (rank == 0) {
    (void)::unlink(path.c_str());
    const std::string tmp = path + ".tmp";
    const int fd = ::open(tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0600);
    if (fd < 0) {
      set_error("rendezvous: cannot create %s", tmp.c_str());
      return VCY_ERR_INVALID_ARG;
    }
    const bool ok = write_all(fd, payload, kRendezvousBytes);
    ::close(fd);
    if (!ok || ::rename(tmp.c_str(), path.c_str()) != 0) {
      set_error("rendezvous: cannot publish %s", path.c_str());
      return VCY_ERR_INTERNAL;
    }
    return VCY_OK;
  }
  const double t_end = now_ms() + timeout_ms;
  while (now_ms() < t_end) {
    const int fd = ::open(path.c_str(), O_RDONLY);
    if (fd >= 0) {
      struct stat st;
      const bool ok = ::fstat(fd, &st) == 0 && (size_t)st.st_size == kRendezvousBytes && read_all(fd, payload, kRendezvousBytes);
      ::close(fd);
      if (ok) return VCY_OK;
    }
    ::usleep(2000);
  }
  set_error("rendezvous: %s did not appear within %d ms", path.c_str(), timeout_ms);
  return VCY_ERR_INTERNAL;
}

// tcp:<host>:<port> -- rank 0 listens on the port and sends the payload to world - 1 connections; the others connect
// (retrying while rank 0 is not listening yet) and read it.
int rendezvous_tcp(const std::string& host, int port, int rank, int world, void* payload, int timeout_ms) {
  const double t_end = now_ms() + timeout_ms;
  if (rank == 0) {
    const int ls = ::socket(AF_INET, SOCK_STREAM, 0);
    if (ls < 0) {
      set_error("rendezvous: socket() failed");
      return VCY_ERR_INTERNAL;
    }
    int one = 1;
    (void)::setsockopt(ls, SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
    sockaddr_in addr{};
    addr.sin_family = AF_INET;
    addr.sin_port = htons((uint16_t)port);
    addr.sin_addr.s_addr = htonl(INADDR_ANY);
    if (::bind(ls, (sockaddr*)&addr, sizeof(addr)) != 0 || ::listen(ls, world) != 0) {
      ::close(ls);
      set_error("rendezvous: cannot listen on port %d", port);
      return VCY_ERR_INVALID_ARG;
    }
    int rc = VCY_OK;
    for (int k = 1; k < world && rc == VCY_OK; ++k) {
      timeval tv;
      const double left = std::max(1.0, t_end - now_ms());
      tv.tv_sec = (long)(left / 1000.0);
      tv.tv_usec = (long)((left - 1000.0 * tv.tv_sec) * 1000.0);
      fd_set fds;
      FD_ZERO(&fds);
      FD_SET(ls, &fds);
      if (::select(ls + 1, &fds, nullptr, nullptr, &tv) <= 0) {
        set_error("rendezvous: %d of %d ranks connected within %d ms", k - 1, world - 1, timeout_ms);
        rc = VCY_ERR_INTERNAL;
        break;
      }
      const int cs = ::accept(ls, nullptr, nullptr);
      if (cs < 0 || !write_all(cs, payload, kRendezvousBytes)) {
        set_error("rendezvous: sending the id failed");
        rc = VCY_ERR_INTERNAL;
      }
      if (cs >= 0) ::close(cs);
    }
    ::close(ls);
    return rc;
  }
  addrinfo hints{}, *res = nullptr;
  hints.ai_family = AF_INET;
  hints.ai_socktype = SOCK_STREAM;
  const std::string port_s = std::to_string(port);
  if (::getaddrinfo(host.c_str(), port_s.c_str(), &hints, &res) != 0 || !res) {
    set_error("rendezvous: cannot resolve %s", host.c_str());
    return VCY_ERR_INVALID_ARG;
  }
  int rc = VCY_ERR_INTERNAL;
  while (now_ms() < t_end) {
    const int cs = ::socket(AF_INET, SOCK_STREAM, 0);
    if (cs < 0) break;
    if (::connect(cs, res->ai_addr, res->ai_addrlen) == 0) {
      const bool ok = read_all(cs, payload, kRendezvousBytes);
      ::close(cs);
      if (ok) {
        rc = VCY_OK;
        break;
      }
    } else {
      ::close(cs);
    }
    ::usleep(5000);
  }
  ::freeaddrinfo(res);
  if (rc != VCY_OK) set_error("rendezvous: no id from %s:%d within %d ms", host.c_str(), port, timeout_ms);
  return rc;
}

int rendezvous(const char* where, int rank, int world, void* payload, int timeout_ms) {
  if (!where || rank < 0 || world < 1 || rank >= world || !payload || timeout_ms <= 0) {
    set_error("rendezvous: invalid argument");
    return VCY_ERR_INVALID_ARG;
  }
  if (world == 1) return VCY_OK;
  const std::string w(where);
  if (w.rfind("file:", 0) == 0 && w.size() > 5) return rendezvous_file(w.substr(5), rank, payload, timeout_ms);
  if (w.rfind("tcp:", 0) == 0) {
    const size_t colon = w.rfind(':');
    if (colon != std::string::npos && colon > 4) {
      const int port = std::atoi(w.c_str() + colon + 1);
      if (port > 0 && port < 65536) return rendezvous_tcp(w.substr(4, colon - 4), port, rank, world, payload, timeout_ms);
    }
  }
  set_error("rendezvous: expected \"file:<path>\" or \"tcp:<host>:<port>\", got \"%s\"", where);
  return VCY_ERR_INVALID_ARG;
}

}  // namespace
}  // namespace vcy

extern "C" int vcy_rendezvous_exchange(int rank, int world, const char* where, void* payload128, int timeout_ms) {
  return vcy::rendezvous(where, rank, world, payload128, timeout_ms);
}
