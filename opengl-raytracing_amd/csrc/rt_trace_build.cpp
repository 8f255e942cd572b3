// rt_trace_build.cpp -- the traversal launches' options and build choice (rt_trace_build.hpp).  getenv, clamps and conditions: no HIP, no context.
#include "rt_trace_build.hpp"

#include <algorithm>
#include <cstdlib>

namespace rtl {

// fused (RT_FUSED=1, measured option of round 5, off): closest-hit launches walk the fused records (DevScene::wF) when rt_upload_bvh built them -- the reference's
// visiting order in half the dependent round trips (bounce rays: 20.6 -> 11.2 steps, primary 17.1 -> 9.7), bit-identical, and 3-4 % SLOWER in every mode (batched,
// frame by frame, one rank of eight): the same number of 16-byte lane-loads per ray, and that number -- not the length of the dependency chain -- is what these
// launches cost (profiles/r05_experiments.txt 1)
TraceTune default_tune() {
    TraceTune t{32, 16, 0, 2, 0, 0, 0, 2, 0, 1, 0, 768, 1, -1, 0, 0, 0};
    if (const char *e = getenv("RT_TRACE_TIMING")) t.timing = atoi(e);
    // impl (RT_IMPLICIT=1, measured option of round 5, off): closest-hit launches walk 48-byte records WITHOUT child references (three loads per node visit instead of
    // four) when every leaf of the tree sits at one depth (rt_upload_bvh) -- bit-identical, 25 % fewer node loads, and no faster (bounce launch 0.615 -> 0.628 ms per
    // frame, primary 0.253 -> 0.259): together with `fused` the second half of the finding that neither the loads nor the dependent steps of these launches can be
    // removed for time while their vector instructions stay (profiles/r05_experiments.txt 2)
    if (const char *e = getenv("RT_IMPLICIT")) t.impl = atoi(e);
    if (const char *e = getenv("RT_FUSED")) t.fused = atoi(e);
    return t;
}
TraceTune tune_from_env() {
    TraceTune t = default_tune();
    if (const char *e = getenv("RT_REFILL_MIN")) t.refillMin = std::max(1, std::min(64, atoi(e)));
    if (const char *e = getenv("RT_CHUNK")) { int v = atoi(e); t.chunk = v <= 0 ? 0 : std::max(8, std::min(1 << 20, v)); }   // 0 = from the queue size
    if (const char *e = getenv("RT_LEAFB")) t.leafb = t.leafbClosest = atoi(e);
    if (const char *e = getenv("RT_LEAFB_CLOSEST")) t.leafbClosest = atoi(e);
    if (const char *e = getenv("RT_MIN_SEARCH")) t.minSearch = std::max(0, std::min(64, atoi(e)));
    if (const char *e = getenv("RT_QUAD_REFILL")) t.quadRefill = atoi(e) != 0;
    if (const char *e = getenv("RT_COOP")) t.coop = atoi(e);   // quad-cooperative node fetch of the closest-hit launches (measured option)
    if (const char *e = getenv("RT_NEAR_FIRST")) t.nearFirst = atoi(e);
    if (const char *e = getenv("RT_REVERSE")) t.reverse = atoi(e);      // 0: any-hit queues dealt from their beginning, as in rounds 1-3
    if (const char *e = getenv("RT_GUIDED")) t.guided = atoi(e);
    if (const char *e = getenv("RT_DENSE_TAKE")) t.denseTake = atoi(e);   // 0: every refill probes liveness first, as in rounds 2-3
    if (const char *e = getenv("RT_QNODES")) t.qnodes = atoi(e);          // 0: never; 1 / 2: always (seven / six waves per SIMD); default: when rt_upload_bvh built them
    return t;
}
int light_masks_from_env() {
    const char *e = getenv("RT_LIGHT_MASKS");
    return e ? std::max(0, std::min(2, atoi(e))) : 1;
}

TraceBuild trace_build(bool any, const TraceTune &tune, const TraceForms &f, int depth, bool stats) {
    TraceBuild b{};
    // Stack entries: closest-hit defers one sibling per binary level (8 B each); any-hit walks 4-wide nodes and can
    // defer three per two levels (4 B each).  Resident 256-thread workgroups per CU follow from the LDS footprint and the kernel's
    // registers: asked from the runtime per (kernel, stack size), the persistent grid is exactly what fits.
    b.stack = std::max(4, any ? (f.anyStack > 0 ? f.anyStack : 3 * ((depth + 1) / 2)) : depth);
    b.ldsBytes = (size_t)256 * b.stack * (any ? 4 : 8);
    // quantised any-hit nodes; qnodes -1: whenever rt_upload_bvh built them (trees beyond the L2).  The diagnostic and near-first builds walk the exact nodes
    const bool qn = any && tune.qnodes != 0 && f.q4 && !stats && !tune.nearFirst;
    // closest-hit launches: the fused records when rt_upload_bvh built them; they yield to COOP
    const bool fuse = !any && tune.fused != 0 && f.wF && !tune.coop;
    // ... the implicit records when every leaf sits at one depth.  Any-hit: with an exact stack, default leaf groups and not the seven-wave quantised build;
    // closest-hit: they yield to the fused records and to COOP.  Of the diagnostic builds only TIMING has an implicit form
    const bool impl = tune.impl != 0 && (!stats || tune.timing) &&
                      (any ? (f.iN4 && (!qn || f.iQ4) && !tune.nearFirst && tune.leafb < 4 && !(qn && tune.qnodes == 1) && f.anyStack > 0) : (!fuse && f.iN2 && !tune.coop));
    b.nodes = any ? (impl ? (qn ? TN_IQ4 : TN_IN4) : (qn ? TN_Q4 : TN_W4)) : (fuse ? TN_WF : (impl ? TN_IN2 : TN_WNODESW));
    b.implPairs = impl;
    b.implLeafBoxes = any && impl;
    const uint32_t leafb4 = (any ? tune.leafb : tune.leafbClosest) >= 4 ? RT_BUILD_LEAFB4 : 0;
    // The precedence of the options, first match wins.  RT_TRACE_TIMING=1: the production kernel of this launch with scalar time stamps (exact / implicit
    // records, default leaf groups only) -- it ignores every other option
    if (stats && tune.timing) b.opt = RT_BUILD_TIMING | (impl ? RT_BUILD_IMPL : 0);
    else if (impl) b.opt = RT_BUILD_IMPL | (qn ? RT_BUILD_QN2 : 0);
    else if (stats) b.opt = RT_BUILD_STATS | (fuse ? RT_BUILD_FUSE : leafb4);
    else if (fuse) b.opt = RT_BUILD_FUSE;
    else if (!any && tune.coop) b.opt = RT_BUILD_COOP;
    else if (any && tune.nearFirst) b.opt = RT_BUILD_NEAR;
    else if (qn) b.opt = tune.qnodes == 1 ? RT_BUILD_QN1 : RT_BUILD_QN2;   // QN1: seven waves per SIMD, 44 B of scratch: slower (measured)
    else b.opt = leafb4;                                                   // (quantised wins over RT_LEAFB=4)
    return b;
}

}  // namespace rtl

// ---- the host-side diagnostics of include/rt_mi355.h
int rt_debug_trace_options(RtTraceOptions *out) {
    if (!out) return RT_ERR_INVALID;
    const rtl::TraceTune t = rtl::tune_from_env();
    *out = RtTraceOptions{t.timing, t.coop, t.nearFirst, t.qnodes, t.fused, t.impl, t.leafb, t.leafbClosest};
    return RT_OK;
}
int rt_debug_trace_build(const RtTraceCase *cases, int64_t n, RtTraceBuild *out) {
    if (!cases || !out || n < 0) return RT_ERR_INVALID;
    for (int64_t i = 0; i < n; ++i) {
        const RtTraceCase &c = cases[i];
        rtl::TraceTune t = rtl::TraceTune{32, 16, 0, 2, 0, 0, 0, 2, 0, 1, 0, 768, 1, -1, 0, 0, 0};   // (the scheduler's fields choose no build)
        t.timing = c.opt.timing; t.coop = c.opt.coop; t.nearFirst = c.opt.nearFirst; t.qnodes = c.opt.qnodes; t.fused = c.opt.fused; t.impl = c.opt.impl;
        t.leafb = c.opt.leafb; t.leafbClosest = c.opt.leafbClosest;
        const rtl::TraceForms f{c.q4 != 0, c.wF != 0, c.iN2 != 0, c.iN4 != 0, c.iQ4 != 0, c.anyStack};
        const rtl::TraceBuild b = rtl::trace_build(c.any != 0, t, f, c.depth, c.stats != 0);
        out[i] = RtTraceBuild{b.opt, (int32_t)b.nodes, b.implPairs ? 1 : 0, b.implLeafBoxes ? 1 : 0, b.stack, 0, (uint64_t)b.ldsBytes};
    }
    return RT_OK;
}
int rt_debug_trace_builds(int any, uint32_t *out, int capacity) {
    const uint32_t *list = any ? rtl::kAnyBuilds : rtl::kClosestBuilds;
    const int n = (int)(any ? rtl::kNAnyBuilds : rtl::kNClosestBuilds);
    for (int i = 0; out && i < n && i < capacity; ++i) out[i] = list[i];
    return n;
}
