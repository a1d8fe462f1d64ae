// host_log2.h -- THE log2 of a size on the host: the smallest k with 2^k >= n (exact for the powers of two every domain size is; 0 for n <= 1).
// Pure host code (no HIP).
#pragma once
#include <cstddef>

namespace kzg {
inline int ilog2_ceil(size_t n) { int k = 0; while (((size_t)1 << k) < n) ++k; return k; }
}  // namespace kzg
