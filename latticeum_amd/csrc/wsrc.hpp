// wsrc.hpp -- where a Witness::from_f_coeff kernel takes its coefficients from: the
// canonical u64 words of f_coeff, or the packed witness payload (lf.h, "witness wire
// format": centred representatives as little-endian i16 / i32, or the residue as u64).
// One kernel body per transform, instantiated per source, as sumcheck.hip does with
// its Pl* digit sources; a packed word is decoded in the register it was loaded into.
#pragma once
#include "digits.hpp"

namespace lfk {

// get(): the coefficient as a canonical field element; bad |= the word is not a valid one
struct SrcU64 {
  using word = uint64_t;
  static constexpr int bits = 64;
  static __device__ __forceinline__ uint64_t get(word w, bool &) { return w; }
};
struct SrcU64Checked {  // a payload word: a residue >= p is refused (and passed on as it is: the call fails)
  using word = uint64_t;
  static constexpr int bits = 64;
  static __device__ __forceinline__ uint64_t get(word w, bool &bad) {
    bad |= w >= gl::P;
    return w;
  }
};
struct SrcI16 {
  using word = int16_t;
  static constexpr int bits = 16;
  static __device__ __forceinline__ uint64_t get(word w, bool &) { return from_signed((int64_t)w); }
};
struct SrcI32 {
  using word = int32_t;
  static constexpr int bits = 32;
  static __device__ __forceinline__ uint64_t get(word w, bool &) { return from_signed((int64_t)w); }
};

// the launchers' runtime name of a source
enum WitnessSrc { WSRC_U64 = 0, WSRC_I16 = 1, WSRC_I32 = 2, WSRC_U64_CHECKED = 3 };

// f(Src{}) for the source `src`
template <class F>
inline hipError_t witness_src(int src, F &&f) {
  switch (src) {
    case WSRC_U64: return f(SrcU64{});
    case WSRC_I16: return f(SrcI16{});
    case WSRC_I32: return f(SrcI32{});
    case WSRC_U64_CHECKED: return f(SrcU64Checked{});
    default: return hipErrorInvalidValue;
  }
}

}  // namespace lfk
