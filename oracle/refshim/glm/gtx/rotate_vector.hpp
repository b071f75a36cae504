// Stand-in for <glm/gtx/rotate_vector.hpp>: rotation of a vec3 about a coordinate axis, in the element type, as GLM's
// manual defines it (the rotated pair is (a*cos - b*sin, a*sin + b*cos) in the axis' right-handed order).
#pragma once
#include <cmath>

#include "../glm.hpp"

namespace glm {
template <typename T>
vec<3, T> rotateX(vec<3, T> const &v, T const &angle) {
  vec<3, T> r(v);
  T const c(std::cos(angle)), s(std::sin(angle));
  r.y = v.y * c - v.z * s;
  r.z = v.y * s + v.z * c;
  return r;
}
template <typename T>
vec<3, T> rotateY(vec<3, T> const &v, T const &angle) {
  vec<3, T> r(v);
  T const c(std::cos(angle)), s(std::sin(angle));
  r.x = v.x * c + v.z * s;
  r.z = -v.x * s + v.z * c;
  return r;
}
template <typename T>
vec<3, T> rotateZ(vec<3, T> const &v, T const &angle) {
  vec<3, T> r(v);
  T const c(std::cos(angle)), s(std::sin(angle));
  r.x = v.x * c - v.y * s;
  r.y = v.x * s + v.y * c;
  return r;
}
}  // namespace glm
