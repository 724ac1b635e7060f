// The one owner of device memory on the host side: every long-lived device pointer of every handle is a DevBuf, so a handle's struct is
// the list of what it owns and its destroy function frees nothing by hand.  Host API only: compiles alone with the host compiler.
//
// A DevBuf's size is only ever the size of the block it holds - there is no capacity kept beside the pointer that could be written
// before an allocation that then fails.  It does not synchronise (callers idle their stream before they drop a buffer that may be in
// flight), does not pool or cache, and does not preserve contents when it grows.
//
// Epochs.  The handles whose buffers a captured graph points into (maua_vgg, maua_secondary, maua_clip, the guides) count buffer
// generations; the one rule: bump the epoch before a buffer such a graph may point into is freed, reallocated or re-placed - a
// failed allocation has moved it too, and the pieces of a carved set move even where their block does not.  Every handle does so in
// the branch that decides to regrow; `moved` (reserve, carve_into, UnitStyles::ensure) is for the caller that cannot know beforehand.
#pragma once
#include <hip/hip_runtime_api.h>

#include "scratch.h"

namespace maua {

class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      free();
      p_ = o.p_; bytes_ = o.bytes_;
      o.p_ = nullptr; o.bytes_ = 0;
    }
    return *this;
  }
  ~DevBuf() { free(); }

  // frees what it holds, then allocates `bytes` (0: a small non-NULL block), zeroed on request.  On failure the buffer is empty.
  int alloc(size_t bytes, bool zero = false) {
    free();
    void* p = nullptr;
    const size_t real = bytes ? bytes : 16;
    hipError_t e = hipMalloc(&p, real);
    if (e == hipSuccess && zero && (e = hipMemset(p, 0, real)) != hipSuccess) (void)hipFree(p);
    if (e != hipSuccess) return fail(std::string("DevBuf: ") + std::to_string(bytes) + " bytes: " + hipGetErrorString(e));
    p_ = p; bytes_ = bytes;
    return MAUA_OK;
  }
  // grow-only alloc: nothing happens while `bytes` fits.  *moved is set whenever the old block was freed (also when the new allocation
  // then fails) and left alone otherwise, so one flag can collect several calls.
  int reserve(size_t bytes, bool* moved = nullptr) {
    if (p_ && bytes <= bytes_) return MAUA_OK;
    if (p_ && moved) *moved = true;
    return alloc(bytes);
  }
  void free() {
    if (p_) (void)hipFree(p_);   // (nothing a caller could do about a failure here)
    p_ = nullptr; bytes_ = 0;
  }
  size_t bytes() const { return bytes_; }
  explicit operator bool() const { return p_ != nullptr; }
  void* get() const { return p_; }
  template <typename T> T* as() const { return (T*)p_; }

 private:
  void* p_ = nullptr;
  size_t bytes_ = 0;
};

// A set of pieces that live, die and regrow together: `layout(Scratch&)` writes the (non-owning) piece pointers, once on a measuring
// Scratch - which leaves them all NULL - and, when `buf` holds that much, once more on the block.  So after a failure the owner is
// empty and every piece is NULL; after success every piece lies in [buf.get(), buf.get() + buf.bytes()) at 256-byte alignment.
template <typename Layout>
int carve_into(DevBuf& buf, Layout&& layout, bool* moved = nullptr) {
  const size_t bytes = scratch_bytes(layout);
  if (bytes == SIZE_MAX) return fail("carve_into: workspace size overflows size_t");
  if (int rc = buf.reserve(bytes, moved)) return rc;
  Scratch place(buf.get());
  layout(place);
  return MAUA_OK;
}

}  // namespace maua
