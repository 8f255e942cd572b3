// rt_beam.hpp -- the beam cull of a batch's primary stage (DESIGN.md 4.2 "Beam cull"): does EVERY primary ray of a screen tile miss the mesh?  Plain C++17, host and
// device, no HIP header: k_beam_cull (rt_wave_stages.hpp) and rt_debug_beam_cull (rt_beam.cpp) evaluate the same functions.  Float model of DESIGN.md 2: nothing
// contracted, fmin / fmax that ignore a NaN operand.
//
// All primary rays of a launch set leave from one origin ro.  slab() (rt_device_shade.hpp) computes per axis fl(c * r), c = fl(b - ro) one float for every ray and r the
// ray's rdInv component.  Rounding is monotone and so are fmin and fmax in each argument: with [L, H] the smallest and largest r any ray of the beam computed, L and H
// finite, normal and of one sign, the kernel's own expressions at L and at H enclose the tmin and the tmax every ray of the beam computes -- the floats, not the real
// numbers.  tmaxHi < tminLo then says that `tmax >= tmin` is false for every ray.  The closest-hit walk enters a node only behind that test of the node's box, so a beam
// whose interval walk leaves no leaf standing holds rays that all miss.  Whatever the argument does not cover keeps the beam: an L or H that is zero, denormal, infinite
// or NaN, L and H of different sign, a bound that is not finite.
#pragma once
#include <cstdint>
#include <cstring>

#ifdef __HIP__
#define RT_BEAM_FN __host__ __device__ inline
#else
#define RT_BEAM_FN inline
#endif

namespace rtbeam {

constexpr int kFrontier = 64;          // inner nodes a level of the walk holds at most: one per lane of a wave
constexpr int kRecordFloats = 16;      // a two-child record: [Lmin.xyz, leftRef] [Lmax.xyz, rightRef] [Rmin.xyz, -] [Rmax.xyz, -]
enum Verdict { kDead = 0, kAlive = 1, kOverflow = 2 };   // kOverflow: kept because a level held more than kFrontier inner nodes

struct Interval { float L[3], H[3]; };   // per axis, the least and the largest rdInv component of the beam's rays

RT_BEAM_FN uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
RT_BEAM_FN float fminb(float a, float b) { return __builtin_fminf(a, b); }
RT_BEAM_FN float fmaxb(float a, float b) { return __builtin_fmaxf(a, b); }
RT_BEAM_FN bool finite_f(float v) { return ((bits_of(v) >> 23) & 0xffu) != 0xffu; }
// finite, normal, not zero: an rdInv component the argument covers
RT_BEAM_FN bool usable(float v) { const uint32_t e = (bits_of(v) >> 23) & 0xffu; return e != 0u && e != 0xffu; }

RT_BEAM_FN void interval_clear(Interval &I) {
    for (int a = 0; a < 3; ++a) { I.L[a] = __builtin_inff(); I.H[a] = -__builtin_inff(); }
}
// one more ray; a component outside the argument poisons its axis for good (no comparison with a NaN is true)
RT_BEAM_FN void interval_add(Interval &I, const float *rdInv) {
    for (int a = 0; a < 3; ++a) {
        const float v = rdInv[a];
        if (!usable(v)) { I.L[a] = I.H[a] = __builtin_nanf(""); continue; }
        if (v < I.L[a]) I.L[a] = v;
        if (v > I.H[a]) I.H[a] = v;
    }
}
// [L, H] per axis over n rdInv triples
RT_BEAM_FN Interval beam_interval(const float *rdInv, int n) {
    Interval I;
    interval_clear(I);
    for (int i = 0; i < n; ++i) interval_add(I, rdInv + (size_t)i * 3);
    return I;
}
RT_BEAM_FN bool interval_ok(const float *L, const float *H) {
    for (int a = 0; a < 3; ++a)
        if (!(usable(L[a]) && usable(H[a]) && L[a] <= H[a] && (L[a] > 0.0f) == (H[a] > 0.0f))) return false;
    return true;
}

// slab() at the interval's ends: out = {tminLo, tminHi, tmaxLo, tmaxHi}, bounds of what the rays of an ok interval compute.  false: the box or the origin is outside
// the argument (a bound that is not finite) and out is not written.
RT_BEAM_FN bool slab_bounds(const float *ro, const float *lo, const float *hi, const float *L, const float *H, float *out) {
    float nLo[3], nHi[3], fLo[3], fHi[3];
    for (int a = 0; a < 3; ++a) {
        const float c0 = lo[a] - ro[a], c1 = hi[a] - ro[a];
        if (!(finite_f(c0) && finite_f(c1))) return false;   // (c == 0, the origin on a plane, gives t = +-0 at both ends; c0 == c1, a flat box, t0 == t1: both covered)
        const float a0 = c0 * L[a], b0 = c0 * H[a], a1 = c1 * L[a], b1 = c1 * H[a];          // t0 and t1 of slab() at both ends
        const float t0Lo = fminb(a0, b0), t0Hi = fmaxb(a0, b0), t1Lo = fminb(a1, b1), t1Hi = fmaxb(a1, b1);
        nLo[a] = fminb(t0Lo, t1Lo); nHi[a] = fminb(t0Hi, t1Hi);                              // fmin(t0, t1)
        fLo[a] = fmaxb(t0Lo, t1Lo); fHi[a] = fmaxb(t0Hi, t1Hi);                              // fmax(t0, t1)
    }
    out[0] = fmaxb(fmaxb(nLo[0], nLo[1]), fmaxb(nLo[2], 0.0f));
    out[1] = fmaxb(fmaxb(nHi[0], nHi[1]), fmaxb(nHi[2], 0.0f));
    out[2] = fminb(fminb(fLo[0], fLo[1]), fLo[2]);
    out[3] = fminb(fminb(fHi[0], fHi[1]), fHi[2]);
    return true;
}
// the same for an interval already found ok: true only when `tmax >= tmin` is false for every ray of the beam
RT_BEAM_FN bool slab_fails_ok(const float *ro, const float *lo, const float *hi, const float *L, const float *H) {
    float b[4];
    return slab_bounds(ro, lo, hi, L, H, b) && b[3] < b[0];
}
RT_BEAM_FN bool beam_slab_fails(const float *ro, const float *lo, const float *hi, const float *L, const float *H) {
    return interval_ok(L, H) && slab_fails_ok(ro, lo, hi, L, H);
}

// child c (0 left, 1 right) of a two-child record: its box and its reference (>= 0 an inner node, < 0 a leaf)
RT_BEAM_FN int child_ref(const float *rec, int c) { return (int)bits_of(rec[c ? 7 : 3]); }
RT_BEAM_FN bool child_fails_ok(const float *rec, int c, const float *ro, const float *L, const float *H) {
    return slab_fails_ok(ro, rec + (c ? 8 : 0), rec + (c ? 12 : 4), L, H);
}

// The interval walk over the two-child records, breadth-first, the frontier at most kFrontier inner nodes: alive as soon as a leaf child survives, kept as soon as
// more than kFrontier inner children survive a level, dead when the frontier empties.  nInner: records in `nodes` (a reference outside them keeps the beam).
// *levels: records' levels walked.  The root's own box is the caller's (beam_cull_tile).
RT_BEAM_FN Verdict beam_walk(const float *nodes, int nInner, int rootRef, const float *ro, const float *L, const float *H, int *levels = nullptr) {
    if (levels) *levels = 0;
    if (!interval_ok(L, H) || rootRef < 0 || rootRef >= nInner) return kAlive;   // (a root that is a leaf: its box survived)
    int cur[kFrontier], next[kFrontier], n = 1;
    cur[0] = rootRef;
    while (n > 0) {
        if (levels) ++*levels;
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const float *rec = nodes + (size_t)cur[i] * kRecordFloats;
            for (int c = 0; c < 2; ++c) {
                if (child_fails_ok(rec, c, ro, L, H)) continue;
                const int ref = child_ref(rec, c);
                if (ref < 0 || ref >= nInner) return kAlive;
                if (m < kFrontier) next[m] = ref;
                ++m;
            }
        }
        if (m > kFrontier) return kOverflow;   // (behind the level's leaves, as the wave decides it: a leaf anywhere in the level says alive)
        for (int i = 0; i < m; ++i) cur[i] = next[i];
        n = m;
    }
    return kDead;
}
// a tile's verdict: the root box first (start_ray's test), then the walk
RT_BEAM_FN Verdict beam_cull_tile(const float *nodes, int nInner, int rootRef, const float *rootMin, const float *rootMax, const float *ro, const Interval &I, int *levels = nullptr) {
    if (levels) *levels = 0;
    if (!interval_ok(I.L, I.H)) return kAlive;
    if (slab_fails_ok(ro, rootMin, rootMax, I.L, I.H)) return kDead;
    return beam_walk(nodes, nInner, rootRef, ro, I.L, I.H, levels);
}

}  // namespace rtbeam
