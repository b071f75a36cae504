// The rounds of a flush of the culled list scan's shared tests in the kernels that fold by minimum (closest_hit.h,
// RUN_TRIS, step (b); kernels.h: pairs_full_rounds).  A pure function of the flush's task count and the threshold, in a
// header of its own that a host program can include alone (tests/test_pair_rounds_host.py does): no HIP, no namespace.
//
// A flush of n_now (ray, pair) tasks is tested by the wave's 64 lanes in rounds.  A PAIR round gives a lane one task,
// both of its triangles: 64 tasks a round.  A TRIANGLE round gives a lane one triangle, two lanes to a task: 32 tasks a
// round, at about two thirds of a pair round's instructions.  So a round that is full either way is cheaper as a pair
// round, and only the short rest of a flush is cheaper in triangles: while more than `pair_min` tasks are untested the
// next round is a pair round over the next 64 (or all that are left); the rest, at most pair_min, goes to triangle
// rounds, which start at triangle 2 * done.
#pragma once

// The next round is a pair round: `done` tasks of the flush's n_now have been tested.
constexpr bool pair_round_due(int n_now, int done, int pair_min) { return n_now - done > pair_min; }

// The schedule written out, for the host: round r covers tasks [first[r], first[r] + count[r]) and is a pair round where
// pair[r] != 0.  Returns the number of rounds (never more than `cap` are written).
inline int pair_round_plan(int n_now, int pair_min, int cap, int *first, int *count, int *pair) {
  int r = 0, done = 0;
  for (; pair_round_due(n_now, done, pair_min); done += 64, r++)  // (the device's loop, statement for statement)
    if (r < cap) first[r] = done, count[r] = n_now - done < 64 ? n_now - done : 64, pair[r] = 1;
  for (int t0 = 2 * done; t0 < 2 * n_now; t0 += 64, r++)  // triangles t0 .. t0 + 63, two to a task
    if (r < cap) first[r] = t0 / 2, count[r] = 2 * n_now - t0 < 64 ? (2 * n_now - t0) / 2 : 32, pair[r] = 0;
  return r;
}
