// The one table from a maua_dtype to sizes, and the one dispatcher from a maua_dtype to an element type.  Plain C++: no HIP header.
#pragma once
#include <stdint.h>
#include <string>
#include <type_traits>

#include "../../include/maua_hip.h"

namespace maua {

int fail(const std::string& msg);  // context.hip: sets the thread-local error, returns MAUA_ERR

// bytes per stored element; 0 for a value that is no maua_dtype (MAUA_F32_SPLIT stores float32: only its products differ)
constexpr int elem_bytes(int dtype) {
  return dtype == MAUA_F32 || dtype == MAUA_F32_SPLIT ? 4 : dtype == MAUA_BF16 || dtype == MAUA_F16 ? 2 : 0;
}
// elements per `bytes`-byte chunk (the 64- and 128-byte K chunks of the GEMM and conv kernels), and per 16-byte piece
constexpr int elems_per_chunk(int dtype, int bytes) { return elem_bytes(dtype) ? bytes / elem_bytes(dtype) : 0; }
constexpr int elems_per_piece(int dtype) { return elems_per_chunk(dtype, 16); }

// the element types kernels are templated on.  bf16_t is raw bfloat16 bits; f16_t (IEEE half) has a type of its own so that a template
// can tell the two 16-bit formats apart; f32s_t is float32 storage whose products run as three split bf16 products.
typedef uint16_t bf16_t;
struct f16_t { uint16_t bits; };
struct f32s_t { float v; };

template <typename T> struct dtype_of;
template <> struct dtype_of<float> { static constexpr int value = MAUA_F32; };
template <> struct dtype_of<bf16_t> { static constexpr int value = MAUA_BF16; };
template <> struct dtype_of<f16_t> { static constexpr int value = MAUA_F16; };
template <> struct dtype_of<f32s_t> { static constexpr int value = MAUA_F32_SPLIT; };

// dispatch_dtype<float, bf16_t>(dtype, "who", [&](auto t) { using T = decltype(t); ... }) calls the callable with a zero of the listed
// type whose dtype this is - so only the listed instantiations exist - and returns its result (MAUA_OK for a callable that returns
// nothing); any other dtype is refused with "who: unsupported dtype".
template <typename... Ts, typename F>
int dispatch_dtype(int dtype, const char* who, F&& f) {
  int rc = MAUA_OK;
  auto call = [&](auto t) {
    if constexpr (std::is_void_v<decltype(f(t))>) f(t);
    else rc = f(t);
    return true;
  };
  if (((dtype == dtype_of<Ts>::value && call(Ts{})) || ...)) return rc;
  return fail(std::string(who) + ": unsupported dtype");
}

}  // namespace maua
