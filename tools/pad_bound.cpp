// pad_bound.cpp — how far from a sphere can the fp32 hit test (trace.hip's
// exact op sequence) report a candidate?  Drives the BVH box padding.
// For random spheres/rays it measures, over fp32 candidates with t > tmin:
//   e_disc = |disc32 - disc_exact| / max(|oc|, r)^2
//   e_pt   = distance from O + t32*u (exact) to the sphere's AABB / (|oc| + r),
//            and / (t + 3 r): the same bound by the hit distance (an accepted
//            body has |oc| <= t + sqrt(3) (r + e)), bvh_pad.h's per-distance form
// One trial in eight leaves the body it tests (the origin an fp32 hit point on
// it, sq = |h|: the self-hit guard's root t = 2 h), reported apart.  That root
// lies exactly as far from the centre as the origin does (|X - C| = |O - C|),
// so it inherits the origin's own offset from the surface -- the earlier
// segment's error, which no bound in this segment's t or |oc| covers.  The
// walk does not need it to: a box is skipped only if its interval misses
// (tmin, t], and the chord's midpoint O + h u, at sqrt(|oc|^2 - h^2) from the
// centre, is inside the body whenever the body is a candidate (disc >= 0), to
// the rounding of disc.  So for this case the figure that matters is how far
// the midpoint lies outside the box.
// g++ -O2 -ffp-contract=off -mfma tools/pad_bound.cpp -o /tmp/pad_bound && /tmp/pad_bound
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>

int main(int argc, char** argv) {
  const long trials = argc > 1 ? std::atol(argv[1]) : 40000000;
  std::mt19937_64 g(12345);
  std::uniform_real_distribution<double> U(-1, 1);
  double max_edisc = 0, max_ept = 0, max_ept_abs_over_D = 0, max_ept_over_t3r = 0;
  double max_self_over_D = 0, max_self_over_t3r = 0, max_mid_over_t3r = 0;
  long cands = 0, self_cands = 0;
  for (long it = 0; it < trials; ++it) {
    // scene-like magnitudes: centres within +-S, origin within +-S (some far), radius log-uniform
    const double S = (it % 10 == 0) ? 1000.0 : 30.0;
    float cx = float(U(g) * 30), cy = float(U(g) * 3), cz = float(U(g) * 30);
    float r = float(std::exp(std::log(0.05) + (U(g) * 0.5 + 0.5) * std::log(40.0)));
    float ox = float(U(g) * S), oy = float(U(g) * S * 0.1 + 1), oz = float(U(g) * S);
    // aim near the sphere silhouette to stress tangency
    double ax = cx - ox + U(g) * r * 1.2, ay = cy - oy + U(g) * r * 1.2, az = cz - oz + U(g) * r * 1.2;
    // the self-hit case: the origin becomes the fp32 hit point of that ray
    // on the body (p = o + t u, one fma per component, as the kernel makes
    // it), the new direction a random one into the body
    const bool self = it % 8 == 7;
    if (self) {
      const float dx0 = float(cx - ox + U(g) * r * 0.9), dy0 = float(cy - oy + U(g) * r * 0.9),
                  dz0 = float(cz - oz + U(g) * r * 0.9);
      const float l0 = std::sqrt(std::fmaf(dz0, dz0, std::fmaf(dy0, dy0, dx0 * dx0)));
      const float vx = dx0 / l0, vy = dy0 / l0, vz = dz0 / l0;
      const float qx = cx - ox, qy = cy - oy, qz = cz - oz;
      const float h0 = std::fmaf(vz, qz, std::fmaf(vy, qy, vx * qx));
      const float c0 = std::fmaf(qx, qx, std::fmaf(qz, qz, std::fmaf(qy, qy, -(r * r))));
      const float d0 = std::fmaf(h0, h0, -c0);
      if (!(d0 >= 0.0f)) continue;
      const float t0 = h0 - std::sqrt(d0);
      if (!(t0 > 1e-3f * l0)) continue;
      ox = std::fmaf(t0, vx, ox);
      oy = std::fmaf(t0, vy, oy);
      oz = std::fmaf(t0, vz, oz);
      ax = U(g);
      ay = U(g);
      az = U(g);
      if (ax * (double(cx) - ox) + ay * (double(cy) - oy) + az * (double(cz) - oz) < 0) ax = -ax, ay = -ay, az = -az;
    }
    float dx = float(ax), dy = float(ay), dz = float(az);
    const float len = std::sqrt(std::fmaf(dz, dz, std::fmaf(dy, dy, dx * dx)));
    const float ux = dx / len, uy = dy / len, uz = dz / len;
    const float tmin = 1e-3f * len;
    const float nr2 = -(r * r);
    const float ocx = cx - ox, ocy = cy - oy, ocz = cz - oz;
    const float h = std::fmaf(uz, ocz, std::fmaf(uy, ocy, ux * ocx));
    const float c = std::fmaf(ocx, ocx, std::fmaf(ocz, ocz, std::fmaf(ocy, ocy, nr2)));
    const float disc = std::fmaf(h, h, -c);
    if (!(std::fmin(disc, std::fmax(h, -c)) >= 0.0f)) continue;
    const float sq = self ? std::fabs(h) : std::sqrt(disc);
    float t = h - sq;
    if (!(t > tmin)) t = h + sq;
    if (!(t > tmin)) continue;
    ++cands;
    // exact (long double) on the same float inputs
    long double Ux = ux, Uy = uy, Uz = uz;
    long double OCx = (long double)cx - ox, OCy = (long double)cy - oy, OCz = (long double)cz - oz;
    long double He = Ux * OCx + Uy * OCy + Uz * OCz;
    long double oc2 = OCx * OCx + OCy * OCy + OCz * OCz;
    long double Ce = oc2 - (long double)r * r;
    long double De = He * He - Ce;
    const long double scale = oc2 > (long double)r * r ? oc2 : (long double)r * r;
    const double ed = double(std::fabs((long double)disc - De) / scale);
    if (ed > max_edisc) max_edisc = ed;
    // point at t (exact arithmetic) vs the sphere's AABB
    long double px = ox + Ux * t, py = oy + Uy * t, pz = oz + Uz * t;
    auto out = [](long double p, long double lo, long double hi) -> long double {
      return p < lo ? lo - p : (p > hi ? p - hi : 0.0L);
    };
    long double ex = out(px, (long double)cx - r, (long double)cx + r);
    long double ey = out(py, (long double)cy - r, (long double)cy + r);
    long double ez = out(pz, (long double)cz - r, (long double)cz + r);
    double e = double(std::sqrt(ex * ex + ey * ey + ez * ez));
    double D = double(std::sqrt(oc2)) + r;
    const double T3 = double(t) + 3.0 * r;
    if (self) {
      ++self_cands;
      if (e / D > max_self_over_D) max_self_over_D = e / D;
      if (e / T3 > max_self_over_t3r) max_self_over_t3r = e / T3;
      // the chord's midpoint (t = h), against the padding at t = h
      const long double mx = ox + Ux * h, my = oy + Uy * h, mz = oz + Uz * h;
      const long double fx = out(mx, (long double)cx - r, (long double)cx + r);
      const long double fy = out(my, (long double)cy - r, (long double)cy + r);
      const long double fz = out(mz, (long double)cz - r, (long double)cz + r);
      const double em = double(std::sqrt(fx * fx + fy * fy + fz * fz)) / (double(h) + 3.0 * r);
      if (em > max_mid_over_t3r) max_mid_over_t3r = em;
      continue;
    }
    if (e / D > max_ept_abs_over_D) max_ept_abs_over_D = e / D;
    if (e / T3 > max_ept_over_t3r) max_ept_over_t3r = e / T3;
    if (e > max_ept) max_ept = e;
  }
  std::printf("candidates %ld\nmax |disc32-disc| / max(|oc|,r)^2 = %.3g\nmax point-outside-AABB = %.3g (abs)\n"
              "max point-outside-AABB / (|oc|+r) = %.3g\nmax point-outside-AABB / (t+3r) = %.3g\n"
              "self-hit guard (sq = |h|): candidates %ld\n  max point-outside-AABB / (|oc|+r) = %.3g\n"
              "  max point-outside-AABB / (t+3r) = %.3g   (the origin's own offset, see above)\n"
              "  max chord-midpoint-outside-AABB / (h+3r) = %.3g\n",
              cands, max_edisc, max_ept, max_ept_abs_over_D, max_ept_over_t3r, self_cands, max_self_over_D,
              max_self_over_t3r, max_mid_over_t3r);
}
