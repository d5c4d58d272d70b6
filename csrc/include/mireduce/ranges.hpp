// Byte ranges of caller buffers: the overlap test and the in-place rule of the scans, for the launchers
// and the host references alike (no HIP headers).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>

#include "mireduce/error.hpp"

namespace mireduce {

// [x, x + xb) and [y, y + yb) share a byte. A null pointer or an empty range overlaps nothing.
inline bool ranges_overlap(const void* x, size_t xb, const void* y, size_t yb) {
  const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), y0 = reinterpret_cast<uintptr_t>(y);
  return x && y && xb && yb && x0 < y0 + yb && y0 < x0 + xb;
}

// The scans read an element before they store it: out may be in itself when the element sizes es and os
// are equal; any other overlap is an error.
inline void require_in_place_or_disjoint(const char* who, const void* in, size_t in_bytes, size_t es, const void* out,
                                         size_t out_bytes, size_t os) {
  if (ranges_overlap(in, in_bytes, out, out_bytes) && !(in == out && es == os))
    throw Error(std::string(who) + ": out may be in (equal element sizes) but must not overlap it otherwise");
}

}  // namespace mireduce
