// launch.hpp -- host-side launch arithmetic shared by every launcher: the grid
// sizes and the one list of X^d + 1 degrees the library is built for.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include <type_traits>
#include <utility>

namespace lfk {

// blocks of t threads that cover n items
inline unsigned blocks(size_t n, int t) { return (unsigned)((n + t - 1) / t); }
// a grid-stride launch never asks for more than this many blocks
inline unsigned grid_cap(size_t n) { return (unsigned)(n < 65536 ? n : 65536); }

// the X^d + 1 degrees of the LDS transform's kernels (ring.hpp stockham4)
using NegaDegrees = std::integer_sequence<int, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096>;

template <class F, int... D>
inline hipError_t nega_degree_in(int d, F &&f, std::integer_sequence<int, D...>) {
  hipError_t e = hipErrorInvalidValue;  // d is not in the list
  (void)((d == D ? (e = f(std::integral_constant<int, D>{}), true) : false) || ...);
  return e;
}
// f(std::integral_constant<int, d>{}) for a supported degree d, else hipErrorInvalidValue
template <class F>
inline hipError_t nega_degree(int d, F &&f) {
  return nega_degree_in(d, f, NegaDegrees{});
}
inline bool nega_degree_ok(int d) {
  return nega_degree(d, [](auto) { return hipSuccess; }) == hipSuccess;
}

}  // namespace lfk
