// Stand-in for <thrust/sort.h> in the CPU build of the reference: thrust::sort(policy, first, last) is std::sort with
// the elements' own operator<.  thrust::sort promises no order among equal keys and neither does std::sort
// (shared assumptions).
#pragma once
#include <algorithm>

namespace thrust {
struct device_policy {};
static constexpr device_policy device{};

template <typename Policy, typename It>
void sort(const Policy &, It first, It last) {
  std::sort(first, last);
}
}  // namespace thrust
