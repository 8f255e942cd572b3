// rt_query_prep.hip -- the prep kernel of the mesh queries: the one kernel behind rt_query_prep (rt_query_launch.hpp).
#include "rt_query_launch.hpp"

namespace rtd {
namespace {

__global__ void k_query_scene_prep(DevFrame *fr, DevScene sc) {
    if (threadIdx.x == 0) { fr->sc = sc; scene_take_root_box(fr->sc); }
}

}  // namespace
}  // namespace rtd

void rt_query_prep(hipStream_t st, rtd::DevFrame *dFrame, const rtd::DevScene &sc) { hipLaunchKernelGGL(rtd::k_query_scene_prep, dim3(1), dim3(64), 0, st, dFrame, sc); }
