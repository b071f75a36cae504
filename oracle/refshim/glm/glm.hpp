// Stand-in for <glm/glm.hpp> in the CPU build of the reference (oracle/Makefile, _ref/libref.so).  Written from GLM's
// generic (non-SIMD) definitions as its manual and the GLSL specification state them; it shares no text with
// oracle/vecmath.hpp, which it is there to cross-check.  Every function is the scalar closed form, evaluated in the
// written order in the element type:
//   dot(a, b)        tmp = a * b; tmp.x + tmp.y + tmp.z
//   cross(x, y)      (x.y*y.z - y.y*x.z, x.z*y.x - y.z*x.x, x.x*y.y - y.x*x.y)
//   length(v)        sqrt(dot(v, v))
//   inversesqrt(x)   1 / sqrt(x)
//   normalize(v)     v * inversesqrt(dot(v, v))
//   reflect(I, N)    I - N * dot(N, I) * 2
//   refract(I, N, e) k = 1 - e*e*(1 - dot(N,I)^2);  k >= 0 ? e*I - (e*dot(N,I) + sqrt(k))*N : 0   (GLSL 8.5)
//   min(a, b)        b < a ? b : a        max(a, b)   a < b ? b : a
//   clamp(x, lo, hi) min(max(x, lo), hi)
// Vectors are zero-initialised by their default constructor (GLM before 0.9.9, or GLM_FORCE_CTOR_INIT); the render
// never reads a default-constructed vector before writing it.
#pragma once
#include <cmath>
#include <cstddef>
#include <type_traits>

namespace glm {

typedef int length_t;

template <length_t L, typename T>
struct vec;

template <typename T>
struct vec<2, T> {
  T x, y;
  vec() : x(0), y(0) {}
  template <typename A, typename = typename std::enable_if<std::is_arithmetic<A>::value>::type>
  explicit vec(A s) : x(static_cast<T>(s)), y(static_cast<T>(s)) {}
  template <typename A, typename B>
  vec(A a, B b) : x(static_cast<T>(a)), y(static_cast<T>(b)) {}
  template <typename U>
  explicit vec(vec<3, U> const &v);
  template <typename U>
  explicit vec(vec<4, U> const &v);
  static length_t length() { return 2; }
  T &operator[](length_t i) { return (&x)[i]; }
  T const &operator[](length_t i) const { return (&x)[i]; }
};

template <typename T>
struct vec<3, T> {
  T x, y, z;
  vec() : x(0), y(0), z(0) {}
  template <typename A, typename = typename std::enable_if<std::is_arithmetic<A>::value>::type>
  explicit vec(A s) : x(static_cast<T>(s)), y(static_cast<T>(s)), z(static_cast<T>(s)) {}
  template <typename A, typename B, typename C>
  vec(A a, B b, C c) : x(static_cast<T>(a)), y(static_cast<T>(b)), z(static_cast<T>(c)) {}
  template <typename U, typename C>
  vec(vec<2, U> const &v, C c) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)), z(static_cast<T>(c)) {}
  template <typename U>
  explicit vec(vec<4, U> const &v);
  static length_t length() { return 3; }
  T &operator[](length_t i) { return i == 0 ? x : (i == 1 ? y : z); }
  T const &operator[](length_t i) const { return i == 0 ? x : (i == 1 ? y : z); }
  vec &operator+=(vec const &v) {
    x += v.x, y += v.y, z += v.z;
    return *this;
  }
  vec &operator-=(vec const &v) {
    x -= v.x, y -= v.y, z -= v.z;
    return *this;
  }
  vec &operator*=(vec const &v) {
    x *= v.x, y *= v.y, z *= v.z;
    return *this;
  }
  vec &operator*=(T s) {
    x *= s, y *= s, z *= s;
    return *this;
  }
  vec &operator/=(T s) {
    x /= s, y /= s, z /= s;
    return *this;
  }
};

template <typename T>
struct vec<4, T> {
  T x, y, z, w;
  vec() : x(0), y(0), z(0), w(0) {}
  template <typename A, typename = typename std::enable_if<std::is_arithmetic<A>::value>::type>
  explicit vec(A s) : x(static_cast<T>(s)), y(static_cast<T>(s)), z(static_cast<T>(s)), w(static_cast<T>(s)) {}
  template <typename A, typename B, typename C, typename D>
  vec(A a, B b, C c, D d) : x(static_cast<T>(a)), y(static_cast<T>(b)), z(static_cast<T>(c)), w(static_cast<T>(d)) {}
  template <typename U, typename D>
  vec(vec<3, U> const &v, D d)
      : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)), z(static_cast<T>(v.z)), w(static_cast<T>(d)) {}
  static length_t length() { return 4; }
  T &operator[](length_t i) { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
  T const &operator[](length_t i) const { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
};

template <typename T>
template <typename U>
vec<2, T>::vec(vec<3, U> const &v) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)) {}
template <typename T>
template <typename U>
vec<2, T>::vec(vec<4, U> const &v) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)) {}
template <typename T>
template <typename U>
vec<3, T>::vec(vec<4, U> const &v) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)), z(static_cast<T>(v.z)) {}

typedef vec<2, float> vec2;
typedef vec<3, float> vec3;
typedef vec<4, float> vec4;
typedef vec<2, double> dvec2;
typedef vec<3, double> dvec3;
typedef vec<4, double> dvec4;

// ------------------------------------------------------------------ component-wise operators
template <typename T>
vec<2, T> operator+(vec<2, T> const &a, vec<2, T> const &b) { return vec<2, T>(a.x + b.x, a.y + b.y); }
template <typename T>
vec<2, T> operator-(vec<2, T> const &a, vec<2, T> const &b) { return vec<2, T>(a.x - b.x, a.y - b.y); }
template <typename T>
vec<2, T> operator*(vec<2, T> const &a, T s) { return vec<2, T>(a.x * s, a.y * s); }
template <typename T>
vec<2, T> operator*(T s, vec<2, T> const &a) { return vec<2, T>(s * a.x, s * a.y); }
template <typename T>
vec<2, T> operator/(vec<2, T> const &a, T s) { return vec<2, T>(a.x / s, a.y / s); }

template <typename T>
vec<3, T> operator+(vec<3, T> const &a, vec<3, T> const &b) { return vec<3, T>(a.x + b.x, a.y + b.y, a.z + b.z); }
template <typename T>
vec<3, T> operator-(vec<3, T> const &a, vec<3, T> const &b) { return vec<3, T>(a.x - b.x, a.y - b.y, a.z - b.z); }
template <typename T>
vec<3, T> operator-(vec<3, T> const &a) { return vec<3, T>(-a.x, -a.y, -a.z); }
template <typename T>
vec<3, T> operator*(vec<3, T> const &a, vec<3, T> const &b) { return vec<3, T>(a.x * b.x, a.y * b.y, a.z * b.z); }
template <typename T>
vec<3, T> operator*(vec<3, T> const &a, T s) { return vec<3, T>(a.x * s, a.y * s, a.z * s); }
template <typename T>
vec<3, T> operator*(T s, vec<3, T> const &a) { return vec<3, T>(s * a.x, s * a.y, s * a.z); }
template <typename T>
vec<3, T> operator/(vec<3, T> const &a, T s) { return vec<3, T>(a.x / s, a.y / s, a.z / s); }
template <typename T>
vec<3, T> operator/(vec<3, T> const &a, vec<3, T> const &b) { return vec<3, T>(a.x / b.x, a.y / b.y, a.z / b.z); }
template <typename T>
bool operator==(vec<3, T> const &a, vec<3, T> const &b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

template <typename T>
vec<4, T> operator+(vec<4, T> const &a, vec<4, T> const &b) {
  return vec<4, T>(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}
template <typename T>
vec<4, T> operator*(vec<4, T> const &a, T s) { return vec<4, T>(a.x * s, a.y * s, a.z * s, a.w * s); }
template <typename T>
vec<4, T> operator*(vec<4, T> const &a, vec<4, T> const &b) {
  return vec<4, T>(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w);
}

// ------------------------------------------------------------------ scalar functions
template <typename T>
T min(T a, T b) { return (b < a) ? b : a; }
template <typename T>
T max(T a, T b) { return (a < b) ? b : a; }
template <typename T>
T clamp(T x, T lo, T hi) { return min(max(x, lo), hi); }
template <typename T>
T inversesqrt(T x) { return static_cast<T>(1) / std::sqrt(x); }
inline float sqrt(float x) { return std::sqrt(x); }
inline double sqrt(double x) { return std::sqrt(x); }
template <typename T>
T radians(T deg) { return deg * static_cast<T>(0.01745329251994329576923690768489); }

// ------------------------------------------------------------------ vector functions
template <typename T>
vec<3, T> min(vec<3, T> const &a, vec<3, T> const &b) { return vec<3, T>(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z)); }
template <typename T>
vec<3, T> max(vec<3, T> const &a, vec<3, T> const &b) { return vec<3, T>(max(a.x, b.x), max(a.y, b.y), max(a.z, b.z)); }
template <typename T>
vec<3, T> clamp(vec<3, T> const &x, T lo, T hi) {
  return min(max(x, vec<3, T>(lo)), vec<3, T>(hi));
}
template <typename T>
vec<3, T> sqrt(vec<3, T> const &v) { return vec<3, T>(std::sqrt(v.x), std::sqrt(v.y), std::sqrt(v.z)); }

template <typename T>
T dot(vec<2, T> const &a, vec<2, T> const &b) {
  vec<2, T> tmp(a.x * b.x, a.y * b.y);
  return tmp.x + tmp.y;
}
template <typename T>
T dot(vec<3, T> const &a, vec<3, T> const &b) {
  vec<3, T> tmp(a * b);
  return tmp.x + tmp.y + tmp.z;
}
template <typename T>
T dot(vec<4, T> const &a, vec<4, T> const &b) {
  vec<4, T> tmp(a * b);
  return (tmp.x + tmp.y) + (tmp.z + tmp.w);
}
template <typename T>
vec<3, T> cross(vec<3, T> const &x, vec<3, T> const &y) {
  return vec<3, T>(x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y);
}
template <length_t L, typename T>
T length(vec<L, T> const &v) { return std::sqrt(dot(v, v)); }
template <length_t L, typename T>
T distance(vec<L, T> const &a, vec<L, T> const &b) { return length(b - a); }
template <typename T>
vec<3, T> normalize(vec<3, T> const &v) { return v * inversesqrt(dot(v, v)); }
template <typename T>
vec<3, T> reflect(vec<3, T> const &I, vec<3, T> const &N) { return I - N * dot(N, I) * static_cast<T>(2); }
template <typename T>
vec<3, T> refract(vec<3, T> const &I, vec<3, T> const &N, T eta) {
  T const d(dot(N, I));
  T const k(static_cast<T>(1) - eta * eta * (static_cast<T>(1) - d * d));
  return (k >= static_cast<T>(0)) ? (eta * I - (eta * d + std::sqrt(k)) * N) : vec<3, T>(0);
}

// ------------------------------------------------------------------ mat4: four column vectors, m[column][row]
template <typename T>
struct mat4x4 {
  vec<4, T> c[4];
  mat4x4() {}
  explicit mat4x4(T s) {
    for (int i = 0; i < 4; i++) c[i][i] = s;
  }
  vec<4, T> &operator[](length_t i) { return c[i]; }
  vec<4, T> const &operator[](length_t i) const { return c[i]; }
};
typedef mat4x4<float> mat4;

template <typename T>
vec<4, T> operator*(mat4x4<T> const &m, vec<4, T> const &v) {
  // GLM: Mov0 = v[0], Mov1 = v[1]; Mul0 = m[0]*Mov0, Mul1 = m[1]*Mov1; Add0 = Mul0+Mul1; likewise 2 and 3; Add0+Add1
  vec<4, T> const add0 = m[0] * v.x + m[1] * v.y;
  vec<4, T> const add1 = m[2] * v.z + m[3] * v.w;
  return add0 + add1;
}
template <typename T>
mat4x4<T> operator*(mat4x4<T> const &a, mat4x4<T> const &b) {
  mat4x4<T> r;
  for (int j = 0; j < 4; j++) r[j] = a[0] * b[j].x + a[1] * b[j].y + a[2] * b[j].z + a[3] * b[j].w;
  return r;
}

}  // namespace glm
