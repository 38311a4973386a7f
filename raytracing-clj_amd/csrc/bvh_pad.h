// bvh_pad.h — the BVH walk's per-ray box padding and slab test, as plain
// inline functions that compile for the device (trace_kernel.h,
// trace_diag.hip) and for the host (tools/pad_check.cpp, the CPU property
// test's driver): one text for both.
//
// What the padding must cover.  The walk is bit-identical to the scan because
// a box only culls: a body the scan's fp32 test accepts with root t must pass
// the slab test of its own box and of every box around it.  The fp32 test can
// report a point X = O + t u slightly outside the body (tools/pad_bound.cpp):
// per axis X lies at most 6e-4 * (|oc| + r) outside the body's box.
//
//  * The ray-wide form (the fallback).  |oc| + r <= D = |O - c_tree| + R_tree
//    for every tree body, so every box grown by P = 2e-3 * D holds X: a
//    margin of 3.4 on the measured 5.94e-4.
//  * The per-distance form.  X is within delta of the body's box, so
//    |oc| <= t + sqrt(3) (r + delta) and the same measurement reads
//    e <= 5.95e-4 * (t + 3 r) (pad_bound reports both ratios).  With
//    pad(t) = k (t + c0), k = 2e-3, c0 >= 3 r_max over the tree's bodies:
//      b_lo - k (t + c0) <= o' + t u <= b_hi + k (t + c0)        per axis,
//    two half-lines in t.  For u > 0:
//      t >= (b_lo - (o' + k c0)) / (u + k)         (near plane)
//      t <= (b_hi - (o' - k c0)) / (u - k)         (far plane, needs u > k)
//    and mirrored for u < 0: with s = sign(u) the near multiplier is
//    1 / (u + s k), the far one 1 / (u - s k), the offsets o' +- s k c0.
//    The node step keeps its one fma per plane; only the multiplier differs
//    between a child's near and far plane.
//
// The limit on |u|.  The far half-line is an upper bound on t only while
// u - s k has u's sign: a multiplier of the wrong sign would turn it into a
// lower bound, a false miss.  An axis can therefore take the per-distance
// form only if |u| > kPadLimit = 1.5 k: then |u - s k| >= k / 2 in exact
// arithmetic, far more than the subtraction's rounding (6e-8 |u|), so the
// sign holds and both multipliers stay below 1 / (k / 2) = 1000.  Each axis'
// slab is a necessary condition on its own in either form, so the forms
// could be mixed per axis; but a ray with an axis at or below the limit (one
// in a hundred of isotropic directions) keeps the ray-wide form (1 / u held
// to +-1e24, and P) on all three: one choice per ray costs 4 instructions
// per segment, one per axis cost 12 more, and the set-up's instructions are
// what the padding's gain is paid with.
//
// The rounding term.  The slab arithmetic rounds too: o' = o - c, o' +- k c0,
// the product with the multiplier and the fma each lose up to 6e-8 of a
// magnitude up to ~D, and the multiplier itself is good to ~2e-7 (rcp 1 ulp,
// u +- k rounded) of a bound up to ~2 D: about 6e-7 * D in position units,
// whatever r_max is.  So c0 = 3 r_max + kPadRound * D with kPadRound = 2e-3:
// k * kPadRound * D = 4e-6 * D, a margin of about 6 over that rounding, and a
// scene of tiny bodies never gets a padding below it.  (The ray-wide P =
// 2e-3 * D covers the same rounding 3000-fold.)
//
// The body the ray leaves.  Its root is the self-hit guard's t = 2 h, a point
// exactly as far from the centre as the origin is: off the surface by the
// earlier segment's error, which nothing in this segment bounds.  The walk
// does not need that point inside the box, only the box's interval to meet
// (tmin, 2 h]: the chord's midpoint t = h lies inside the body whenever the
// body is a candidate (tools/pad_bound.cpp measures it: never outside the
// box), and the far bounds carry + tmin for the case h < tmin < 2 h.
//
// The other fallback.  If k c0 >= P (a tree with a body about as large as
// the tree itself) the ray keeps the ray-wide form too: never looser than it.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define RT_PAD_FN __host__ __device__ __forceinline__
#else
#define RT_PAD_FN inline
#endif

namespace rtclj {

constexpr float kPadK = 2e-3f;       // k: padding per unit of D (ray-wide) or of t + c0 (per-distance)
constexpr float kPadLimit = 3e-3f;   // per-axis limit on |u| (1.5 k, above)
constexpr float kPadRound = 2e-3f;   // c0's share of D (the slab arithmetic's rounding, above)
constexpr float kPadRmax = 3.0f;     // c0's share of r_max
constexpr float kPadAbs = 5e-4f;     // added to D: a floor of k * kPadAbs = 1e-6 under the ray-wide padding

// host equivalents of the device builtins: 1 ulp apart at most, far inside
// the padding (boxes only cull)
RT_PAD_FN float pad_rcp(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rcpf(x);
#else
  return 1.0f / x;
#endif
}
RT_PAD_FN float pad_sqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_sqrtf(x);
#else
  return std::sqrt(x);
#endif
}
// float <-> bits
RT_PAD_FN unsigned pad_u(float x) { return __builtin_bit_cast(unsigned, x); }
RT_PAD_FN float pad_f(unsigned x) { return __builtin_bit_cast(float, x); }
// m ? a : b per bit (m all ones or all zeros).  On the device one v_bitop3_b32
// (LUT 0xe4 = (s0 & s2) | (s1 & ~s2)): a full-rate op that pairs with its
// neighbour, where v_cndmask_b32 / v_bfi_b32 hold the VALU for a whole cycle
RT_PAD_FN unsigned pad_sel(unsigned m, unsigned a, unsigned b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(a, b, m, 0xe4);
#else
  return (a & m) | (b & ~m);
#endif
}
// v_fma_f32 in its three-address form on the device (the compiler's
// v_fmac_f32 needs a v_mov copy when the addend stays live)
RT_PAD_FN float pad_fma(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
  float r;
  asm("v_fma_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
#else
  return std::fma(a, b, c);
#endif
}

// x & L, x | L, L - x with the literal L inside the instruction (VOP2 takes
// one): a literal the compiler sees three times it keeps in a register through
// the whole walk, and the walk has none to spare
template <unsigned L>
RT_PAD_FN unsigned pad_and(unsigned x) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned r;
  asm("v_and_b32 %0, %1, %2" : "=v"(r) : "n"(L), "v"(x));
  return r;
#else
  return x & L;
#endif
}
template <unsigned L>
RT_PAD_FN unsigned pad_or(unsigned x) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned r;
  asm("v_or_b32 %0, %1, %2" : "=v"(r) : "n"(L), "v"(x));
  return r;
#else
  return x | L;
#endif
}
template <unsigned L>
RT_PAD_FN unsigned pad_rsub(unsigned x) {
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned r;
  asm("v_sub_u32 %0, %1, %2" : "=v"(r) : "n"(L), "v"(x));
  return r;
#else
  return L - x;
#endif
}
// all ones if the integer is negative
RT_PAD_FN unsigned pad_neg_mask(unsigned x) { return static_cast<unsigned>(static_cast<int>(x) >> 31); }

// The set-up runs once per segment for all 64 lanes, so it is written in ops
// that issue at full rate and in pairs (add, mul, and, or, shifts, v_bitop3
// -- DESIGN.md 5.1) where a compare and a select would each hold the VALU for
// a whole cycle: a choice is a mask made by an integer subtraction and an
// arithmetic shift, and a sign is moved by and / or.

// per ray: which form its three axes take, and that form's constants
struct PadRay {
  float p;          // the padding's constant part: k c0 (per-distance) or P = k D' (ray-wide)
  unsigned kn, kf;  // bits of what s adds to u for the near and the far multiplier:
                    // k and -k (per-distance), or 1e-24 for both (ray-wide, below)
  unsigned per_t;   // all ones: per-distance
};
// (ex, ey, ez) = O - c_tree, (ux, uy, uz) the unit direction, R the tree's
// bounding radius, c0_bodies = kPadRmax * r_max of the tree's bodies (the
// host's figure, KArgs::bvh_c0)
RT_PAD_FN PadRay pad_ray(float ex, float ey, float ez, float ux, float uy, float uz, float R, float c0_bodies,
                         bool allow_per_t = true) {
  constexpr unsigned kLimBits = __builtin_bit_cast(unsigned, kPadLimit), kKBits = __builtin_bit_cast(unsigned, kPadK),
                     kTinyBits = __builtin_bit_cast(unsigned, 1e-24f);
  // D' = D + kPadAbs: an absolute floor of k * kPadAbs = 1e-6 under either
  // padding (as an add before the product: each op takes its literal itself;
  // k D + 1e-6 as one fma holds a constant in a register)
  const float D = pad_sqrt(fmaf(ez, ez, fmaf(ey, ey, ex * ex))) + R + kPadAbs;
  const float P = kPadK * D;
  const float pc = kPadK * fmaf(kPadRound, D, c0_bodies);
  PadRay r;
  // per-distance if pc < P and every |u| component is above the limit.
  // Positive floats order like their bits, so each answer is the sign of an
  // integer difference (all below 2^31).
  const float umin = fminf(fminf(fabsf(ux), fabsf(uy)), fabsf(uz));
  r.per_t = allow_per_t ? pad_neg_mask(pad_u(pc) - pad_u(P)) & pad_neg_mask(pad_rsub<kLimBits>(pad_u(umin))) : 0u;
  r.p = pad_f(pad_sel(r.per_t, pad_u(pc), pad_u(P)));
  // ray-wide: u moved away from zero by 1e-24 (its own sign) for both
  // planes: nothing at all above 1e-17, and below it a 1/u of at most 1e24
  // -- with u = 0 an infinite 1/u makes the fma bounds NaN and -inf, which
  // would collapse the slab (a false miss); finite, the slab of an origin
  // inside the padded box spans ~+-1e24 and one outside it lies ~1e24 away
  // (culled) -- the u = 0 answers.  (u = -0 gives -1e24: the sign still
  // orders the planes.)
  r.kn = kTinyBits + (pad_and<kKBits - kTinyBits>(r.per_t));
  r.kf = r.kn ^ pad_and<0x80000000u>(r.per_t);
  return r;
}

// one axis of a ray: plane b (relative to the tree centre) is met at
// t = b * m + o, with (mn, on) for the near plane and (mf, of) for the far one
struct PadAxis {
  float mn, mf, on, of;
  unsigned sign;   // u's sign bit (0x80000000: the box's max plane is the near one)
};
// u: the unit direction's component, e: the origin's, relative to the tree
// centre; tmin: the segment's lower bound on t
RT_PAD_FN PadAxis pad_axis(float u, float e, float tmin, const PadRay& r) {
  PadAxis a;
  a.sign = pad_and<0x80000000u>(pad_u(u));
  // 1 / (u + s k) and 1 / (u - s k), or 1 / (u + s 1e-24) twice (kn > 0: s
  // goes in by or; kf has a sign of its own: by xor)
  const unsigned skn = a.sign | r.kn;
  a.mn = pad_rcp(u + pad_f(skn));
  a.mf = pad_rcp(u + pad_f(a.sign ^ r.kf));
  // the near plane is the min plane for u >= 0 (offset o' + p), the max
  // plane for u < 0 (offset o' - p); the far plane the other one
  const float sp = pad_f(a.sign | pad_u(r.p));   // (p >= 0)
  a.on = -(e + sp) * a.mn;
  // the far bound carries + tmin (the product's fma: no instruction more),
  // for the body the ray leaves: the guard's root t = 2 h is accepted if
  // 2 h > tmin, and what the box is known to hold is the chord's midpoint
  // t = h (inside the body whenever disc >= 0), which may lie below tmin;
  // with tf >= h + tmin the interval still meets (tmin, 2 h]
  a.of = fmaf(-(e - sp), a.mf, tmin);
  return a;
}

// one box: its (near, far) planes per axis -> the entry and exit t
RT_PAD_FN void pad_interval(const PadAxis& x, const PadAxis& y, const PadAxis& z, float xn, float xf, float yn,
                            float yf, float zn, float zf, float& tn, float& tf) {
  const float tnx = pad_fma(xn, x.mn, x.on), tfx = pad_fma(xf, x.mf, x.of);
  const float tny = pad_fma(yn, y.mn, y.on), tfy = pad_fma(yf, y.mf, y.of);
  const float tnz = pad_fma(zn, z.mn, z.on), tfz = pad_fma(zf, z.mf, z.of);
  tn = fmaxf(fmaxf(tnx, tny), tnz);
  tf = fminf(fminf(tfx, tfy), tfz);
}

// the cull predicate "[tn, tf] meets (tmin, best_t]" as tn <= min(tf, best_t)
// and tmin <= tf (tmin < best_t always).  Each is "not greater", so a NaN
// bound passes (conservative).
RT_PAD_FN bool pad_meets(float tn, float tf, float tmin, float best_t) {
  float tb;
#if defined(__HIP_DEVICE_COMPILE__)
  // (a bare v_min_f32: fminf would re-canonicalise best_t every step; a NaN
  // tf gives best_t, conservative)
  asm("v_min_f32 %0, %1, %2" : "=v"(tb) : "v"(tf), "v"(best_t));
#else
  tb = tf < best_t ? tf : best_t;   // (a NaN tf gives best_t)
#endif
  return !(tn > tb) & !(tmin > tf);
}

}  // namespace rtclj
