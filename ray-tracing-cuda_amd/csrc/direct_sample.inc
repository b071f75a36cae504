// SAMPLE of rtmi_direct_sample / rtmi_direct_sample_mis, as a fragment of text (direct_weigh.inc says why a fragment):
// the draws from the path's light state, the light picked, the point or direction on it, validity, the weighted
// contribution and the shadow ray.  Included by direct_body.h and by render_body.h in its DIRECT mode.
//
// In scope at the site: bool MIS, SPH, staged;  const float *s_cdf;  const LightTable &lt;  and, written here:
// V3 x (the vertex), wi (the shadow direction, zero when invalid), dir (the contribution);  float t_max;  bool valid.
// As macros: RTMI_DS_STATE(k) (word k of the path's light state, an lvalue), RTMI_DS_ORIGIN (V3: the vertex),
// RTMI_DS_HIT_N (V3: the hit record's normal), RTMI_DS_ATTENUATION (V3: the vertex's attenuation).
          Rng rng;
          rng.d = RTMI_DS_STATE(0), rng.v0 = RTMI_DS_STATE(1);
          rng.v1 = RTMI_DS_STATE(2), rng.v2 = RTMI_DS_STATE(3);
          rng.v3 = RTMI_DS_STATE(4), rng.v4 = RTMI_DS_STATE(5);
          const float r0 = rng_range(0.f, 1.f, rng);
          float r1 = rng_range(0.f, 1.f, rng);
          float r2 = 0.f;
          if constexpr (!SPH) {
            r2 = rng_range(0.f, 1.f, rng);
            RTMI_DS_STATE(0) = rng.d, RTMI_DS_STATE(1) = rng.v0;
            RTMI_DS_STATE(2) = rng.v1, RTMI_DS_STATE(3) = rng.v2;
            RTMI_DS_STATE(4) = rng.v3, RTMI_DS_STATE(5) = rng.v4;
          }
          const int j = staged ? light_pick(s_cdf, lt.n_lights, r0) : light_pick(lt.cdf, lt.n_lights, r0);
          const float4 *lp = reinterpret_cast<const float4 *>(lt.recs + j);
          const float4 l0 = lp[0], l1 = lp[1], l2 = lp[2], l3 = lp[3];  // p0 e1.x | e1.yz e2.xy | e2.z n | emission scale
          const int4 l4 = reinterpret_cast<const int4 *>(lt.recs + j)[4];
          const V3 N = RTMI_DS_HIT_N;
          bool sph = false;
          if constexpr (SPH) {
            // a sphere light takes r1 and a point of the unit disc by rejection (the Lambertian ball sampler's kind of loop:
            // no trip cap), every draw before any validity test; a flat light takes r2 as ever
            sph = l4.x == 2;
            float cp = 0.f, sp = 0.f;
            if (sph) {
              float da, db, s2d;
              do {
                da = rng_range(-1.f, 1.f, rng);
                db = rng_range(-1.f, 1.f, rng);
                s2d = da * da + db * db;
              } while (!(s2d > 0.f && s2d <= 1.f));
              const float ls = sqrtf(s2d);
              cp = da / ls, sp = db / ls;
            } else {
              r2 = rng_range(0.f, 1.f, rng);
            }
            RTMI_DS_STATE(0) = rng.d, RTMI_DS_STATE(1) = rng.v0;
            RTMI_DS_STATE(2) = rng.v1, RTMI_DS_STATE(3) = rng.v2;
            RTMI_DS_STATE(4) = rng.v3, RTMI_DS_STATE(5) = rng.v4;
            if (sph) {
              x = RTMI_DS_ORIGIN;
              const float R2 = l1.x;
              const SphereCone k = sphere_cone(mk(l0.x, l0.y, l0.z), R2, x);
              const float dc = sqrtf(k.d2c);
              const float h = r1 * k.om;
              const float ct = 1.f - h;
              const float st2 = h * (2.f - h);
              const float st = sqrtf(st2);
              // the cone's axis and Duff et al.'s branch-free frame around it
              const V3 w = k.wc / dc;
              const float sg = w.z >= 0.f ? 1.f : -1.f;
              const float ka = -1.f / (sg + w.z);
              const float kb = (w.x * w.y) * ka;
              const V3 u = mk(1.f + (sg * (w.x * w.x)) * ka, sg * kb, (-sg) * w.x);
              const V3 v = mk(kb, sg + (w.y * w.y) * ka, -w.y);
              const float sc = st * cp, ss = st * sp;
              wi = (ct * w + sc * u) + ss * v;
              // the near intersection of that direction with the sphere
              const float tc = dc * ct;
              float q = R2 - k.d2c * st2;
              q = q > 0.f ? q : 0.f;
              const float t = tc - sqrtf(q);
              const float cs = dot3(N, wi);
              valid = k.outside && cs > 0.f && t > 0.f && t < INFINITY;
              if (valid) {
                const float av = (cs * k.om) * l3.w;
                float g = av;
                if constexpr (MIS) g = av / (av + 1.f);
                const V3 att = RTMI_DS_ATTENUATION;
                dir = (att * mk(l3.x, l3.y, l3.z)) * g;
                t_max = t * 0.999f;
              } else {
                wi = splat(0.f);
              }
            }
          }
          if (!sph) {
            if (l4.x == 1 && r1 + r2 > 1.f) r1 = 1.f - r1, r2 = 1.f - r2;
            const V3 p0 = mk(l0.x, l0.y, l0.z), e1 = mk(l0.w, l1.x, l1.y), e2 = mk(l1.z, l1.w, l2.x), ln = mk(l2.y, l2.z, l2.w);
            const V3 q = (p0 + r1 * e1) + r2 * e2;
            x = RTMI_DS_ORIGIN;
            const V3 w = q - x;
            const float d2 = dot3(w, w);
            const float dist = sqrtf(d2);
            wi = w / dist;
            const float cs = dot3(N, wi);
            const float cl = fabsf(dot3(ln, wi));
            valid = d2 > 0.f && cs > 0.f && cl > 0.f && dist < INFINITY;
            if (valid) {
              float g;
              if constexpr (MIS) {
                const float av = (cs * cl) * l3.w;
                g = av / (av + d2);
              } else {
                g = ((cs * cl) / d2) * l3.w;
              }
              const V3 att = RTMI_DS_ATTENUATION;
              dir = (att * mk(l3.x, l3.y, l3.z)) * g;
              t_max = dist * 0.999f;
            } else {
              wi = splat(0.f);
            }
          }
