// Stand-in for <glm/gtc/constants.hpp>: the decimal expansions GLM's manual gives, narrowed once to T.
#pragma once
#include "../glm.hpp"

namespace glm {
template <typename T>
constexpr T pi() { return static_cast<T>(3.14159265358979323846264338327950288); }
template <typename T>
constexpr T two_pi() { return static_cast<T>(6.28318530717958647692528676655900576); }
template <typename T>
constexpr T half_pi() { return static_cast<T>(1.57079632679489661923132169163975144); }
}  // namespace glm
