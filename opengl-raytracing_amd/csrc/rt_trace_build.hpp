// rt_trace_build.hpp -- what a traversal launch (rt_trace.hpp) decides before it launches, without a device: the scheduler's tunables and
// the switches of the environment, and from them, the node forms the scene offers and the tree's depth the k_trace build -- named by its RT_BUILD_* bits
// (include/rt_mi355.h) --, the node array it walks, its stack and its LDS bytes.  No HIP, no context: launch_trace follows the choice, rt_debug_trace_build
// hands it out without a GPU.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/rt_mi355.h"

namespace rtl {

// Tunables of the scheduler (overridable per context through RT_REFILL_MIN / RT_MIN_SEARCH for experiments).  A kernel argument: the layout is k_trace's.
struct TraceTune { int refillMin; int minSearch; int chunk; int leafb; int skipTraversal; int quadRefill; int coop; int leafbClosest; int nearFirst; int reverse; int guided; int chunkMax; int denseTake; int qnodes; int fused; int impl; int timing; };   // skipTraversal: diagnostic (RT_DEBUG_SKIP_TRAVERSAL)
TraceTune default_tune();
// default_tune() with the scheduler and kernel-build options of the environment: what a context's frames launch (rt_wave_create) and what rt_debug_trace
// kinds 2 - 4 launch (rt_wave_debug_trace / rt_wave_debug_packets), so that the per-ray tests walk the build a frame walks under the same environment.
// RT_DEBUG_SKIP_TRAVERSAL is not read here: it skips the work, and only frames take it.
TraceTune tune_from_env();
// RT_LIGHT_MASKS: 1 (default) the light slots of shadow queue 1 are marked live in bit masks instead of by tMax words < 0; 2 (measured option)
// those of shadow queue 2 as well; 0 neither, the A/B switch.
// Read beside tune_from_env, not into TraceTune: that record is an argument of every k_trace build, and a member more would move the arguments behind it in all of them.
int light_masks_from_env();

// What a scene offers a launch: the optional record forms rt_upload_bvh built (DevScene's pointers, non-null) and the exact any-hit stack size (0: not known)
struct TraceForms { bool q4, wF, iN2, iN4, iQ4; int anyStack; };

// The node array a launch walks (DevScene's member of the same name)
enum TraceNodes { TN_WNODESW = RT_TRACE_NODES_WNODESW, TN_WF = RT_TRACE_NODES_WF, TN_IN2 = RT_TRACE_NODES_IN2, TN_W4 = RT_TRACE_NODES_W4, TN_Q4 = RT_TRACE_NODES_Q4,
                  TN_IN4 = RT_TRACE_NODES_IN4, TN_IQ4 = RT_TRACE_NODES_IQ4 };

struct TraceBuild {
    uint32_t opt;          // the build: an OR of RT_BUILD_LEAFB4 .. RT_BUILD_TIMING, unshifted and without RT_BUILD_LAUNCHED -- k_trace's OPT
    TraceNodes nodes;
    bool implPairs;        // the pair records are iPairs, not pairs
    bool implLeafBoxes;    // the leaf boxes are iLeafBox, not leafBox
    int stack;             // stack entries per lane
    size_t ldsBytes;       // dynamic LDS of a 256-thread workgroup: its stacks
};
// any: any-hit launch (4-byte stack entries, the 4-wide nodes).  depth: of the binary tree.  stats: the launch was given sums to add to (RT_TRACE_STATS / RT_TRACE_TIMING).
// k_trace_packets launches with the any-hit stack and LDS bytes of this function (it walks w4 whatever the tune says).
TraceBuild trace_build(bool any, const TraceTune &tune, const TraceForms &forms, int depth, bool stats);

// The k_trace builds the library holds, per hit kind: every `opt` trace_build can return is one of them (tests/test_trace_build_host.py walks the whole
// domain), and launch_trace instantiates exactly these.
constexpr uint32_t kClosestBuilds[] = {0, RT_BUILD_LEAFB4, RT_BUILD_STATS, RT_BUILD_LEAFB4 | RT_BUILD_STATS, RT_BUILD_COOP, RT_BUILD_FUSE, RT_BUILD_STATS | RT_BUILD_FUSE,
                                       RT_BUILD_IMPL, RT_BUILD_TIMING, RT_BUILD_IMPL | RT_BUILD_TIMING};
constexpr uint32_t kAnyBuilds[] = {0, RT_BUILD_LEAFB4, RT_BUILD_STATS, RT_BUILD_LEAFB4 | RT_BUILD_STATS, RT_BUILD_NEAR, RT_BUILD_QN1, RT_BUILD_QN2, RT_BUILD_IMPL,
                                   RT_BUILD_QN2 | RT_BUILD_IMPL, RT_BUILD_TIMING, RT_BUILD_IMPL | RT_BUILD_TIMING};
constexpr size_t kNClosestBuilds = sizeof kClosestBuilds / sizeof kClosestBuilds[0], kNAnyBuilds = sizeof kAnyBuilds / sizeof kAnyBuilds[0];

}  // namespace rtl
