// rt_qnode.hpp -- the one quantiser of four-wide any-hit nodes.  Host C++ (rt_scene_pack.cpp: the explicit and the implicit records of an
// upload) and device code (rt_mesh.hip k_mesh_nodes4: a rebuild or refit) call the same expressions, so the three forms agree bit for bit by construction.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define RT_HD __host__ __device__
#else
#define RT_HD
#endif
#ifndef RT_NO_CHILD
#define RT_NO_CHILD 0x7fffffff   // rt_device_shade.hpp
#endif

// o: the 24 floats of a four-wide record, component-wise [min.x x4][min.y x4][min.z x4][max.x x4][max.y x4][max.z x4]; ref: its four child references
// (RT_NO_CHILD: absent, its box is not looked at).  Writes pieces 0-2 of the quantised record into q[0..11]
//   piece 0: origin.xyz (float), biased exponents ex | ey << 8 | ez << 16       piece 1: lo.x lo.y lo.z hi.x, one byte per child
//   piece 2: hi.y hi.z - -
// and returns whether every decoded box -- in the kernel's own expression fmaf(byte, 2^e, origin) -- contains its child's.  false: q is not to be used.
// Origin = the children's common minimum, one power-of-two step per axis, bytes moved outward until the decoded box contains the child's.
RT_HD inline bool rt_quantise_node4(const float *o, const int *ref, uint32_t *q) {
    for (int k = 0; k < 12; ++k) q[k] = 0u;
    float org[3], scale[3];
    uint32_t exps = 0;
    for (int a = 0; a < 3; ++a) {
        float lo = __builtin_inff(), hi = -__builtin_inff();
        for (int i = 0; i < 4; ++i)
            if (ref[i] != RT_NO_CHILD) { const float l = o[4 * a + i], h = o[12 + 4 * a + i]; lo = l < lo ? l : lo; hi = hi < h ? h : hi; }   // std::min / std::max
        if (!(lo <= hi)) { lo = hi = 0.0f; }
        int eb = 1;
        const double ext = ((double)hi - (double)lo) / 255.0;
        // frexp's exponent from the double's bits: ext > 0 is a difference of floats (>= 2^-149) divided by 255, a positive normal double (or +inf, which
        // the range check below rejects as it rejects every step beyond 2^127)
        if (ext > 0.0) { const int e2 = (int)((__builtin_bit_cast(uint64_t, ext) >> 52) & 0x7ff) - 1022; eb = e2 - 1 + 127 > 1 ? e2 - 1 + 127 : 1; }
        // (the search ends after a step or two: kept scalar, or the host compiler evaluates sixteen candidate steps per round of a vectorised loop)
#pragma clang loop vectorize(disable) interleave(disable)
        while (eb <= 254 && __builtin_fmaf(255.0f, __builtin_bit_cast(float, (uint32_t)eb << 23), lo) < hi) ++eb;
        if (eb > 254) return false;
        org[a] = lo; scale[a] = __builtin_bit_cast(float, (uint32_t)eb << 23);   // 2^(eb - 127), from the exponent field
        exps |= (uint32_t)eb << (8 * a);
        q[a] = __builtin_bit_cast(uint32_t, lo);
    }
    q[3] = exps;
    bool ok = true;
    for (int i = 0; i < 4; ++i) {
        if (ref[i] == RT_NO_CHILD) continue;
        for (int a = 0; a < 3; ++a) {
            const float lo = o[4 * a + i], hi = o[12 + 4 * a + i];
            int ql = (int)__builtin_floor(((double)lo - (double)org[a]) / (double)scale[a]);
            ql = ql < 255 ? ql : 255; ql = ql > 0 ? ql : 0;
            while (ql > 0 && __builtin_fmaf((float)ql, scale[a], org[a]) > lo) --ql;
            int qh = (int)__builtin_ceil(((double)hi - (double)org[a]) / (double)scale[a]);
            qh = qh < 255 ? qh : 255; qh = qh > 0 ? qh : 0;
            while (qh < 255 && __builtin_fmaf((float)qh, scale[a], org[a]) < hi) ++qh;
            if (__builtin_fmaf((float)ql, scale[a], org[a]) > lo || __builtin_fmaf((float)qh, scale[a], org[a]) < hi) ok = false;
            const int wl = 4 + a, wh = a == 0 ? 7 : 7 + a;      // words: lo.x lo.y lo.z hi.x | hi.y hi.z
            q[wl] |= (uint32_t)ql << (8 * i);
            q[wh] |= (uint32_t)qh << (8 * i);
        }
    }
    return ok;
}
