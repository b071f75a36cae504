// Stand-in for <curand_kernel.h> in the CPU build of the reference.  curandState is the XORWOW state; curand_init and
// curand_uniform forward to oracle/xorwow.hpp, the restatement that oracle/rocrand_xcheck.cc pins bit for bit to
// rocRAND's generator (recurrence, Weyl step, 2^67 sequence jump).  The seed salts stay as published in cuRAND's header.
#pragma once
#include <cstdint>

#include "../xorwow.hpp"

struct curandStateXORWOW {
  unsigned int d, v[5];
  int boxmuller_flag;
  int boxmuller_flag_double;
  float boxmuller_extra;
  double boxmuller_extra_double;
};
typedef curandStateXORWOW curandState;
typedef curandStateXORWOW curandState_t;

inline void curand_init(unsigned long long seed, unsigned long long subsequence, unsigned long long offset,
                        curandState *state) {
  orc::Xorwow x = orc::xorwow_init(seed, subsequence);
  for (unsigned long long i = 0; i < offset; i++) orc::xorwow_next(&x);
  state->d = x.d;
  for (int i = 0; i < 5; i++) state->v[i] = x.v[i];
  state->boxmuller_flag = 0;
  state->boxmuller_flag_double = 0;
  state->boxmuller_extra = 0.f;
  state->boxmuller_extra_double = 0.;
}

inline unsigned int curand(curandState *state) {
  orc::Xorwow x;
  x.d = state->d;
  for (int i = 0; i < 5; i++) x.v[i] = state->v[i];
  unsigned int r = orc::xorwow_next(&x);
  state->d = x.d;
  for (int i = 0; i < 5; i++) state->v[i] = x.v[i];
  return r;
}

// (0, 1]: x * 2^-32 + 2^-33
inline float curand_uniform(curandState *state) {
  return (float)curand(state) * 2.3283064e-10f + (2.3283064e-10f / 2.0f);
}
