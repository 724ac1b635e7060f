// The one carver of a one-shot workspace into 256-byte aligned pieces.  Plain C++: no HIP header.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string>

#include "../../include/maua_hip.h"

namespace maua {

int fail(const std::string& msg);                                     // context.hip
int scratch_reserve(maua_ctx* ctx, size_t bytes, void** base);  // context.hip: grows ctx's arena (synchronising) when too small

constexpr size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Scratch(nullptr) measures, Scratch(base) places: a layout is one function of a Scratch, run once for the size and once for the
// pointers, so the two cannot disagree.  bytes() is what was taken - every piece rounded up to 256 bytes, nothing else.
class Scratch {
 public:
  explicit Scratch(void* base = nullptr) : base_((char*)base) {}
  template <typename T> T* take(size_t count) {
    if (count > (SIZE_MAX - 255) / sizeof(T) || align256(count * sizeof(T)) > SIZE_MAX - off_) {
      ok_ = false;   // the byte size does not fit a size_t: refuse, and stay refused
      return nullptr;
    }
    T* p = base_ ? (T*)(base_ + off_) : nullptr;
    off_ += align256(count * sizeof(T));
    return p;
  }
  size_t bytes() const { return off_; }
  bool ok() const { return ok_; }

 private:
  char* base_;
  size_t off_ = 0;
  bool ok_ = true;
};

// what `layout(Scratch&, args...)` takes (SIZE_MAX if that overflows): the size an exported *_workspace function reports for the layout
// its entry point then places
template <typename Layout, typename... Args>
size_t scratch_bytes(Layout&& layout, Args... args) {
  Scratch measure;
  layout(measure, args...);
  return measure.ok() ? measure.bytes() : SIZE_MAX;
}

// the shared arena of a context: measure `layout`, reserve that much, run `layout` again on the arena
template <typename Layout>
int carve_scratch(maua_ctx* ctx, Layout&& layout) {
  const size_t bytes = scratch_bytes(layout);
  if (bytes == SIZE_MAX) return fail("scratch: workspace size overflows size_t");
  void* base = nullptr;
  if (int rc = scratch_reserve(ctx, bytes, &base)) return rc;
  Scratch place(base);
  layout(place);
  return MAUA_OK;
}

}  // namespace maua
