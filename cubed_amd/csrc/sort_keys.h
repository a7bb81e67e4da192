// sort_keys.h -- the key order shared by sort.hip and search.hip.
//
// Keys are f32, f64, i32, i64, u32 or u64.  Ascending, with every NaN above
// every number and all NaNs tied; -0.0 and 0.0 tie.
#pragma once
#include "common.h"

namespace cubed {

template <typename T>
constexpr bool is_float_key = is_same_v<T, float> || is_same_v<T, double>;

// a sorts before b (ascending)
template <typename T>
CUBED_DEV bool key_lt(T a, T b) {
  if constexpr (is_float_key<T>) return a < b || (b != b && a == a);
  else return a < b;
}

}  // namespace cubed
