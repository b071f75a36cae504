// The candidates of a list, as every wavefront entry takes them (rtmi_bounce_list, rtmi_path_compact, rtmi_direct_sample,
// rtmi_direct_sample_mis, rtmi_occluded_list, rtmi_path_advance), and THE statement of the list rule:
//
//   the list ends at  end = min(n_list, *count)   (count null: n_list -- the device's word cuts the host's bound short,
//                                                  never the other way);
//   entry e < end is  list ? list[e] : e          (a null list is the identity);
//   an entry that is no path (>= n) is dropped before anything is addressed with it.
//
// The range tests (e < end, entry < n) stay at the sites: folded into one predicate here they changed the instructions
// of both path_advance_kernels and both direct kernels.  Two sites restate the first two lines in their own text, because
// the helpers moved their kernels: render_body.h's LIST branch (bounce_list_kernel<18>) and occlusion_body.h's
// (all eight occlusion_list_kernel<F>, whose end is formed in 64 bits).  DESIGN.md 2.18, NOTES.md "One path list".
#pragma once
// (included inside namespace rtmi; needs nothing but <stdint.h>)

struct PathList {
  const uint32_t *list;   // nullable: entry e of the list is path list[e] (null: path e)
  const uint32_t *count;  // nullable: a device word that cuts the list short
  uint32_t n_list;        // the host's bound on the list's length (capi.hip: at most 2^31 - 1)
};

__device__ __forceinline__ uint32_t list_end(const PathList &l) {
  uint32_t end = l.n_list;
  if (l.count) {
    const uint32_t c = *l.count;
    end = c < end ? c : end;
  }
  return end;
}

__device__ __forceinline__ uint32_t list_entry(const PathList &l, uint32_t e) { return l.list ? l.list[e] : e; }
