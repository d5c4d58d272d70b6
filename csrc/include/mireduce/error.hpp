// The exception library code throws (check.hpp has the macros that raise it). On its own, without the
// HIP headers, so that host-only headers can throw it too.
#pragma once

#include <stdexcept>

namespace mireduce {

// Library code throws (so the Python binding can turn errors into exceptions); apps use the
// *_FATAL forms which print and exit like the reference.
struct Error : std::runtime_error {
  using std::runtime_error::runtime_error;
};

}  // namespace mireduce
