// Stand-alone check of maua_amd/csrc/devbuf.h (the one owner of device memory, and the carved-set helper) with a host compiler and no
// HIP runtime: hipMalloc / hipFree / hipMemset / hipGetErrorString are defined here over malloc, with a count of live blocks and a
// switch that makes the k-th allocation fail (tests/test_devbuf_host.py compiles it with the address and undefined-behaviour
// sanitizers and runs it).  Exit status 0 and "ok" on stdout when every check holds; the first failing check is named on stderr.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>

#include "maua_hip.h"
#include "devbuf.h"
#include "scratch.h"

static std::string g_err;
int maua::fail(const std::string& msg) {
  g_err = msg;
  return MAUA_ERR;
}

static int g_live = 0;        // blocks allocated and not freed
static int g_calls = 0;       // hipMalloc calls so far
static int g_fail_at = -1;    // the call (counted from 0) that fails; -1: none
static size_t g_last = 0;     // bytes of the last successful allocation

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
  if (g_calls++ == g_fail_at) {
    *p = nullptr;
    return hipErrorOutOfMemory;
  }
  *p = std::aligned_alloc(256, (bytes + 255) & ~(size_t)255);
  if (!*p) return hipErrorOutOfMemory;
  std::memset(*p, 0xAB, bytes);
  g_live++;
  g_last = bytes;
  return hipSuccess;
}
hipError_t hipFree(void* p) {
  if (p) {
    g_live--;
    std::free(p);
  }
  return hipSuccess;
}
hipError_t hipMemset(void* p, int v, size_t bytes) {
  std::memset(p, v, bytes);
  return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "out of memory (test)"; }
}

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);        \
      return 1;                                                      \
    }                                                                \
  } while (0)

using namespace maua;

struct Set { float* a = nullptr; char* b = nullptr; double* c = nullptr; };
static bool inside(const DevBuf& buf, const void* p, size_t bytes) {
  const char *lo = buf.as<char>(), *q = (const char*)p;
  return q >= lo && q + bytes <= lo + buf.bytes() && (size_t)(q - lo) % 256 == 0;
}

static int run() {
  // ---- alloc / reserve / free: live blocks, sizes, zeroing
  DevBuf a;
  CHECK(!a && a.get() == nullptr && a.bytes() == 0 && g_live == 0);
  CHECK(a.alloc(100) == MAUA_OK && a && a.bytes() == 100 && g_live == 1);
  CHECK(a.alloc(300, true) == MAUA_OK && a.bytes() == 300 && g_live == 1);   // (frees what it held)
  for (int i = 0; i < 300; i++) CHECK(a.as<unsigned char>()[i] == 0);
  CHECK(a.alloc(0) == MAUA_OK && a && a.bytes() == 0 && g_live == 1 && g_last == 16);   // zero bytes: a small non-NULL block
  a.free();
  CHECK(!a && a.bytes() == 0 && g_live == 0);
  a.free();   // (twice is fine)
  CHECK(g_live == 0);

  // ---- reserve grows only: a smaller size neither moves nor reallocates
  bool moved = false;
  CHECK(a.reserve(1000, &moved) == MAUA_OK && !moved && a.bytes() == 1000 && g_live == 1);   // nothing was held: nothing moved
  void* const at = a.get();
  const int calls = g_calls;
  CHECK(a.reserve(10, &moved) == MAUA_OK && a.reserve(1000, &moved) == MAUA_OK && a.reserve(0, &moved) == MAUA_OK);
  CHECK(!moved && a.get() == at && a.bytes() == 1000 && g_calls == calls && g_live == 1);
  CHECK(a.reserve(1001, &moved) == MAUA_OK && moved && a.bytes() == 1001 && g_live == 1);
  DevBuf none;
  CHECK(none.reserve(0) == MAUA_OK && none && none.bytes() == 0 && g_live == 2);   // an empty buffer reserves even zero bytes
  none.free();

  // ---- a failed reserve leaves the buffer empty, reports the move, and the same size succeeds later
  moved = false;
  g_fail_at = g_calls;
  CHECK(a.reserve(5000, &moved) == MAUA_ERR && moved && a.get() == nullptr && a.bytes() == 0 && !a && g_live == 0);
  CHECK(g_err.find("5000") != std::string::npos);
  g_fail_at = -1;
  moved = false;
  CHECK(a.reserve(5000, &moved) == MAUA_OK && !moved && a.bytes() == 5000 && g_live == 1);
  g_fail_at = g_calls;
  CHECK(a.alloc(64) == MAUA_ERR && !a && a.bytes() == 0 && g_live == 0);
  g_fail_at = -1;

  // ---- moves: the source is emptied, the target's old block is freed
  CHECK(a.alloc(64) == MAUA_OK && g_live == 1);
  void* const held = a.get();
  DevBuf b(std::move(a));
  CHECK(!a && a.get() == nullptr && a.bytes() == 0 && b.get() == held && b.bytes() == 64 && g_live == 1);
  DevBuf c;
  CHECK(c.alloc(32) == MAUA_OK && g_live == 2);
  c = std::move(b);
  CHECK(!b && b.bytes() == 0 && c.get() == held && c.bytes() == 64 && g_live == 1);
  DevBuf& self = c;
  c = std::move(self);
  CHECK(c.get() == held && g_live == 1);
  {
    DevBuf scoped;
    CHECK(scoped.alloc(8) == MAUA_OK && g_live == 2);
  }
  CHECK(g_live == 1);   // the destructor frees
  c.free();
  CHECK(g_live == 0);

  // ---- the carved set: every piece inside the block at 256-byte alignment ...
  Set s;
  DevBuf ws;
  size_t na = 3, nb = 257, nc = 40;
  auto layout = [&](Scratch& sc) { s.a = sc.take<float>(na); s.b = sc.take<char>(nb); s.c = sc.take<double>(nc); };
  moved = false;
  const size_t measured = scratch_bytes(layout);   // (measuring runs the layout: it leaves every piece NULL)
  CHECK(measured == 256 + 512 + 512 && s.a == nullptr && s.b == nullptr && s.c == nullptr);
  CHECK(carve_into(ws, layout, &moved) == MAUA_OK && !moved && g_live == 1 && ws.bytes() == measured);
  CHECK(inside(ws, s.a, na * 4) && inside(ws, s.b, nb) && inside(ws, s.c, nc * 8));
  std::memset(s.a, 1, na * 4); std::memset(s.b, 2, nb); std::memset(s.c, 3, nc * 8);   // (sanitizer: all of it is ours)
  // ... a smaller set is placed in the same block
  void* const ws_at = ws.get();
  na = 1; nb = 1; nc = 1;
  CHECK(carve_into(ws, layout, &moved) == MAUA_OK && !moved && ws.get() == ws_at && ws.bytes() == 1280);
  CHECK((void*)s.a == ws_at && s.b == (char*)ws_at + 256 && (char*)s.c == (char*)ws_at + 512);
  // ... and when the allocation of a larger one fails the owner is empty and no piece points anywhere: the next call of the same
  // shape cannot take a stale size for a workspace
  na = 1000; nb = 1000; nc = 1000;
  g_fail_at = g_calls;
  CHECK(carve_into(ws, layout, &moved) == MAUA_ERR && moved && !ws && ws.bytes() == 0 && g_live == 0);
  CHECK(s.a == nullptr && s.b == nullptr && s.c == nullptr);
  g_fail_at = -1;
  moved = false;
  CHECK(carve_into(ws, layout, &moved) == MAUA_OK && !moved && ws.bytes() == 4096 + 1024 + 8192 && g_live == 1);
  CHECK(inside(ws, s.a, na * 4) && inside(ws, s.b, nb) && inside(ws, s.c, nc * 8));

  // ---- a layout whose size overflows size_t is refused without an allocation
  const int before = g_calls;
  void* const kept = ws.get();
  auto huge = [&](Scratch& sc) { s.a = sc.take<float>(16); s.c = sc.take<double>(SIZE_MAX / 8 + 1); };
  CHECK(carve_into(ws, huge, &moved) == MAUA_ERR && g_calls == before && !moved && ws.get() == kept && g_live == 1);
  CHECK(g_err.find("overflows") != std::string::npos && s.a == nullptr && s.c == nullptr);
  return 0;
}

int main() {
  if (int rc = run()) return rc;
  CHECK(g_live == 0);   // every owner of run() has gone: nothing is left
  std::puts("ok");
  return 0;
}
