// rt_scene_query.hip -- the analytic leg of the scene queries (rt_trace_scene_rays, rt_pick_pixels): one lane per ray through
// traceAnalyticCore (rt_scene_analytic.glsl:132-167), the frame's scene query of the analytic scene, inlined.  Its answers go straight into the
// caller's outputs; in BVH and hybrid modes the mesh leg (SceneSrc, rt_wave.hip) then walks the uploaded BVH and merges its answers into them.
#define RT_ANALYTIC_LEAF __forceinline__   // as calls (the header's default) every Hit would live in scratch memory (rt_device_analytic.hpp)
#include "rt_device_analytic.hpp"
#include "rt_wave.hpp"

#include "../../include/rt_mi355.h"

#pragma clang fp contract(off)

namespace rtd {

static_assert(RT_OBJECT_FLOOR == MAT_FLOOR && RT_OBJECT_ALBEDO_SPHERE == MAT_ALBEDO_SPHERE && RT_OBJECT_GLASS_SPHERE == MAT_GLASS_SPHERE &&
                  RT_OBJECT_MIRROR_SPHERE == MAT_MIRROR_SPHERE && RT_OBJECT_POINT_LIGHT == MAT_POINTLIGHT_SPHERE && RT_OBJECT_MESH == MAT_MESH,
              "RT_OBJECT_* are the device's material ids");

// Ray i of the query: the caller's arrays, or the primary ray of pixel (x, y) exactly as the frame builds it (rt_mega.hip, primaryDirK of rt_wave.hip).
RT_DEV void scene_ray(const RtUniforms &u, const SceneRays &r, uint32_t i, V3 &ro, V3 &rd) {
    if (r.xy) {
        ro = ld3(u.camPos);
        rd = primaryDirJ(u, (float)r.xy[(size_t)i * 2] + 0.5f, (float)r.xy[(size_t)i * 2 + 1] + 0.5f, u.jitter[0], u.jitter[1]);
    } else {
        ro = ld3(r.o + (size_t)i * r.os);
        rd = ld3(r.d + (size_t)i * r.ds);
    }
}

// ANY: occluded[i] = (analytic t <= tMax[i]); else the closest analytic answer if its t <= tMax[i] (no tMax: any hit), a miss otherwise.  ANALYTIC false
// (BVH mode): every answer a miss / not occluded, for the mesh leg to overwrite.  Block 0 also writes the query scratch the mesh leg reads.
template <bool ANY, bool ANALYTIC>
__global__ __launch_bounds__(256) void k_scene_analytic(const RtUniforms u, DevScene sc, int flags, SceneRays r, DevFrame *fr, uint32_t *head, uint32_t nHead) {
    if (blockIdx.x == 0) {
        for (uint32_t k = threadIdx.x; k < nHead; k += blockDim.x) head[k] = 0u;
        const uint32_t *src = reinterpret_cast<const uint32_t *>(&u);
        uint32_t *dst = reinterpret_cast<uint32_t *>(&fr->u);
        for (uint32_t k = threadIdx.x; k < sizeof(RtUniforms) / 4; k += blockDim.x) dst[k] = src[k];
        if (threadIdx.x == 0) { fr->sc = sc; scene_take_root_box(fr->sc); }
    }
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= r.n) return;
    const float tMax = r.tm ? r.tm[i] : u.inf;
    Hit h;
    h.t = u.inf;
    bool hit = false;
    if (ANALYTIC && !(r.tm && tMax < 0.0f)) {
        V3 ro, rd;
        scene_ray(u, r, i, ro, rd);
        Work w;
        hit = traceAnalyticCore<false>(u, ro, rd, (flags & RT_QUERY_SKIP_GLASS) == 0, (flags & RT_QUERY_SKIP_MARKER) == 0, h, w);
        if (r.tm) hit = hit && h.t <= tMax;
    }
    if (ANY) {
        r.occ[i] = hit ? 1 : 0;
        return;
    }
    r.hits[i] = hit ? make_float4(h.t, __int_as_float(-1), 0.0f, 0.0f) : make_float4(u.inf, __int_as_float(-1), 0.0f, 0.0f);
    if (r.objects) r.objects[i] = hit ? h.mat : RT_OBJECT_NONE;
    const V3 n = hit ? h.n : mk3(0.0f), p = hit ? h.p : mk3(0.0f);
    if (r.normals) { r.normals[(size_t)i * 3] = n.x; r.normals[(size_t)i * 3 + 1] = n.y; r.normals[(size_t)i * 3 + 2] = n.z; }
    if (r.points) { r.points[(size_t)i * 3] = p.x; r.points[(size_t)i * 3 + 1] = p.y; r.points[(size_t)i * 3 + 2] = p.z; }
}

}  // namespace rtd

using namespace rtd;

void rt_scene_query_analytic(hipStream_t st, const RtUniforms &u, const DevScene &sc, int flags, const SceneRays &r, DevFrame *dFrame, uint32_t *heads) {
    const unsigned blocks = std::max(1u, (r.n + 255u) / 256u);
    const bool any = r.hits == nullptr, analytic = u.useBVH != 1;
    const uint32_t nHead = (uint32_t)rt_wave_head_words();
    if (any && analytic) hipLaunchKernelGGL((k_scene_analytic<true, true>), dim3(blocks), dim3(256), 0, st, u, sc, flags, r, dFrame, heads, nHead);
    else if (any) hipLaunchKernelGGL((k_scene_analytic<true, false>), dim3(blocks), dim3(256), 0, st, u, sc, flags, r, dFrame, heads, nHead);
    else if (analytic) hipLaunchKernelGGL((k_scene_analytic<false, true>), dim3(blocks), dim3(256), 0, st, u, sc, flags, r, dFrame, heads, nHead);
    else hipLaunchKernelGGL((k_scene_analytic<false, false>), dim3(blocks), dim3(256), 0, st, u, sc, flags, r, dFrame, heads, nHead);
}
