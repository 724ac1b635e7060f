// Stand-alone check of maua_amd/csrc/dtype.h and scratch.h with a host compiler: no HIP header, no library (tests/test_dtype_scratch_host.py
// compiles and runs it).  Exit status 0 and "ok" on stdout when every check holds; the first failing check is named on stderr.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "maua_hip.h"
#include "dtype.h"
#include "scratch.h"

static std::string g_err;
int maua::fail(const std::string& msg) {
  g_err = msg;
  return MAUA_ERR;
}

#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);        \
      return 1;                                                      \
    }                                                                \
  } while (0)

using namespace maua;

struct Odd { char c[7]; };   // a 7-byte element: odd byte sizes

// one mixed layout, run once to measure and once to place
struct Pieces { float* a; char* b; double* none; Odd* c; uint16_t* d; char* e; };
static Pieces layout(Scratch& s) {
  return Pieces{s.take<float>(3), s.take<char>(257), s.take<double>(0), s.take<Odd>(37), s.take<uint16_t>(128), s.take<char>(1)};
}

int main() {
  // ---- the table
  const int dtypes[4] = {MAUA_F32, MAUA_BF16, MAUA_F16, MAUA_F32_SPLIT}, bytes[4] = {4, 2, 2, 4};
  for (int i = 0; i < 4; i++) {
    CHECK(elem_bytes(dtypes[i]) == bytes[i]);
    CHECK(elems_per_piece(dtypes[i]) == 16 / bytes[i]);
    CHECK(elems_per_chunk(dtypes[i], 64) == 64 / bytes[i] && elems_per_chunk(dtypes[i], 128) == 128 / bytes[i]);
  }
  for (int bad : {4, -1}) CHECK(elem_bytes(bad) == 0 && elems_per_piece(bad) == 0 && elems_per_chunk(bad, 64) == 0);
  static_assert(elem_bytes(MAUA_F32_SPLIT) == 4 && elems_per_piece(MAUA_BF16) == 8, "the table is constexpr");
  static_assert(sizeof(float) == 4 && sizeof(bf16_t) == 2 && sizeof(f16_t) == 2 && sizeof(f32s_t) == 4, "element types have the table's sizes");

  // ---- the dispatcher: the listed types only, the callable's result, the refusal's text
  int seen = -1;
  auto size_of = [&](auto t) { seen = (int)sizeof(t) * 10 + (std::is_same_v<decltype(t), f16_t> ? 1 : 0); return 7; };
  CHECK((dispatch_dtype<float, bf16_t, f16_t>(MAUA_F16, "who", size_of)) == 7 && seen == 21);
  CHECK((dispatch_dtype<float, bf16_t, f16_t>(MAUA_BF16, "who", size_of)) == 7 && seen == 20);
  CHECK((dispatch_dtype<float, bf16_t, f16_t>(MAUA_F32, "who", size_of)) == 7 && seen == 40);
  seen = -1;
  CHECK((dispatch_dtype<float, bf16_t, f16_t>(MAUA_F32_SPLIT, "who", size_of)) == MAUA_ERR && seen == -1 && g_err == "who: unsupported dtype");
  CHECK((dispatch_dtype<float, bf16_t>(MAUA_F16, "op", size_of)) == MAUA_ERR && g_err == "op: unsupported dtype");
  CHECK((dispatch_dtype<f32s_t>(-1, "op", size_of)) == MAUA_ERR && seen == -1);
  CHECK((dispatch_dtype<bf16_t, float>(MAUA_F32, "op", [&](auto t) { seen = (int)sizeof(t); })) == MAUA_OK && seen == 4);   // a void callable

  // ---- the carver
  CHECK(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512);
  Scratch measure;
  const Pieces m = layout(measure);
  CHECK(measure.ok() && !m.a && !m.b && !m.none && !m.c && !m.d && !m.e);
  // 12 -> 256, 257 -> 512, 0 -> 0, 259 -> 512, 256 -> 256, 1 -> 256
  CHECK(measure.bytes() == 256 + 512 + 0 + 512 + 256 + 256);
  CHECK(scratch_bytes(layout) == measure.bytes());
  char* base = (char*)std::aligned_alloc(256, measure.bytes());
  CHECK(base);
  Scratch place(base);
  const Pieces p = layout(place);
  CHECK(place.ok() && place.bytes() == measure.bytes());
  const char* ptrs[6] = {(char*)p.a, p.b, (char*)p.none, (char*)p.c, (char*)p.d, p.e};
  const size_t offs[6] = {0, 256, 768, 768, 1280, 1536};   // the zero-count piece takes no room: it shares its successor's offset
  for (int i = 0; i < 6; i++) CHECK(ptrs[i] == base + offs[i] && (size_t)(ptrs[i] - base) % 256 == 0);
  for (size_t i = 0; i < measure.bytes(); i++) base[i] = 1;   // every byte handed out lies inside the allocation (sanitizer builds)
  std::free(base);

  // ---- overflow: refused, never wrapped, and the carver stays refused
  Scratch big;
  CHECK(big.take<char>(100) == nullptr && big.ok());
  CHECK(big.take<double>(SIZE_MAX / 8 + 1) == nullptr && !big.ok());            // count * 8 wraps
  Scratch big2;
  CHECK(big2.take<char>(SIZE_MAX - 100) == nullptr && !big2.ok());               // the round-up to 256 wraps
  static char room[1024];
  Scratch big3(room);
  big3.take<char>(512);
  CHECK(big3.take<char>(SIZE_MAX - 511) == nullptr && !big3.ok() && big3.bytes() == 512);   // the running total wraps
  CHECK(big3.take<char>(1) != nullptr && !big3.ok());
  CHECK(scratch_bytes([](Scratch& s) { s.take<float>(SIZE_MAX / 2); }) == SIZE_MAX);
  std::puts("ok");
  return 0;
}
