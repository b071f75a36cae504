// WEIGH of rtmi_direct_sample_mis, as a fragment of text: included where a function body has the hit and the path's flag
// at hand, once by direct_body.h (the wavefront step) and once by render_body.h in its DIRECT mode (rtmi_trace_direct), so that the
// rule exists once.  A fragment, not a __device__ function: a function shared between kernels changes the instructions of
// the ones that exist (path_shared.h says what it did), text that the preprocessor pastes does not.
//
// In scope at the site: bool SPH;  int32_t kind, entry, face (the hit's);  uint32_t or bool `was` (the flag as the last
// vertex left it);  const LightTable &lt;  bool dropped (set when an emission is weighed).  As macros, each evaluated where
// it stands: RTMI_DS_HIT_LIGHT, RTMI_DS_N_ENTRIES (the hit -> light map), RTMI_DS_HIT_T (the hit's t), RTMI_DS_ORIGIN (V3:
// the vertex the ray left), RTMI_DS_CARRY (float4), RTMI_DS_EMITTED (V3) and RTMI_DS_EMITTED_SET(x, y, z).
          // WEIGH: the light of the hit by its entry (and face), every index checked before it addresses anything
          int32_t col = -1;
          if (kind == QHIT_PARALLELEPIPED) col = face >= 0 && face < kHitLightAny ? face : -1;
          else if (kind == QHIT_TRIANGLE || kind == QHIT_PARALLELOGRAM) col = kHitLightAny;
          if constexpr (SPH)
            if (kind == QHIT_SPHERE) col = kHitLightAny;
          int32_t j = -1;
          if (was && col >= 0 && entry >= 0 && entry < RTMI_DS_N_ENTRIES) j = RTMI_DS_HIT_LIGHT[(int64_t)entry * kHitLightCols + col];
          bool flat = true;
          if constexpr (SPH) {
            if (kind == QHIT_SPHERE) {
              flat = false;
              if (j >= 0 && j < lt.n_lights && reinterpret_cast<const int4 *>(lt.recs + j)[4].x == 2) {
                const float4 *lp = reinterpret_cast<const float4 *>(lt.recs + j);
                const float4 l0 = lp[0], l1 = lp[1], l3 = lp[3];  // c R | R2 .. | emission scale
                const SphereCone k = sphere_cone(mk(l0.x, l0.y, l0.z), l1.x, RTMI_DS_ORIGIN);
                if (k.outside) {
                  const float av = (RTMI_DS_CARRY.w * k.om) * l3.w;
                  const float sum = av + 1.f;
                  const bool div = av > 0.f && sum < INFINITY;
                  const float w = av / sum;
                  const V3 e = RTMI_DS_EMITTED;
                  RTMI_DS_EMITTED_SET(div ? e.x * w : 0.f, div ? e.y * w : 0.f, div ? e.z * w : 0.f);
                  dropped = true;
                }
              }
            }
          }
          if (flat && j >= 0 && j < lt.n_lights) {
            const float4 c = RTMI_DS_CARRY;
            const float4 *lp = reinterpret_cast<const float4 *>(lt.recs + j);
            const float4 l2 = lp[2], l3 = lp[3];  // e2.z n | emission scale
            const float cl = fabsf(dot3(mk(l2.y, l2.z, l2.w), mk(c.x, c.y, c.z)));
            const float t = RTMI_DS_HIT_T;
            const float d2 = t * t;
            const float av = (c.w * cl) * l3.w;
            const float sum = av + d2;
            const bool div = av > 0.f && d2 > 0.f && sum < INFINITY;
            const float w = av / sum;
            const V3 e = RTMI_DS_EMITTED;
            RTMI_DS_EMITTED_SET(div ? e.x * w : 0.f, div ? e.y * w : 0.f, div ? e.z * w : 0.f);
            dropped = true;
          }
