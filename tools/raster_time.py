"""Times rt_render_raster (device ms from rt_get_raster_stats, and wall ms per frame over back-to-back calls).

    python tools/raster_time.py [--frames N] [--out profiles/raster_time.json]

Cases: renderRaster's scene at 1920x1080 (2-triangle ground quad, bunny stand-in of 81 920 triangles, UV sphere, point-light marker)
with the default and the close-up camera (and the default camera once more with bin arrays for half of its pairs, so that half of
the triangles take the path past the capacity), and the 1 M-triangle scene of BASELINE configs[4] drawn as one mesh with the identity model.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import opengl_raytracing_amd as rt  # noqa: E402
from opengl_raytracing_amd import meshgen  # noqa: E402
import scenes  # noqa: E402


def case(ren, name, draws, cam, frames, W, H):
    view, proj = rt.camera_view(cam), rt.camera_proj(cam)
    for _ in range(3):
        ren.render_raster(draws, view, proj)          # warm-up: sizes the bin arrays
    dev = []
    for _ in range(frames):
        ren.render_raster_async(draws, view, proj)
        dev.append(ren.raster_stats().deviceMs)
    ren.synchronize()
    t0 = time.perf_counter()
    for _ in range(frames):
        ren.render_raster_async(draws, view, proj)
    ren.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / frames
    st = ren.raster_stats()
    r = {"case": name, "size": [W, H], "frames": frames, "device_ms_median": float(np.median(dev)), "device_ms_min": float(np.min(dev)),
         "wall_ms_per_frame": wall, "triangles_in": st.trianglesIn, "set_up": st.trianglesSetUp, "dropped": st.trianglesDropped,
         "clipped": st.trianglesClipped, "bin_entries": st.binEntries, "bin_capacity": st.binCapacity, "raster_bytes": st.rasterBytes}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    W, H = 1920, 1080
    out = []
    with rt.Renderer() as ren:
        ren.resize(W, H)
        b = meshgen.bunny_standin(6)
        s = meshgen.uv_sphere(32, 16)
        g = np.array([[-20, 0, -20], [20, 0, -20], [20, 0, 20], [-20, 0, 20]], np.float32), np.array([0, 2, 1, 0, 3, 2], np.uint32)
        ren.raster_mesh(0, *g)
        ren.raster_mesh(1, b[0], b[1])
        ren.raster_mesh(2, s[0], s[1])
        draws = rt.raster_scene_draws(rt.default_render_params(), 0, 1, 2)
        for cam in ("default", "closeup"):
            out.append(case(ren, f"renderRaster scene, {cam} camera", draws, scenes.camera(cam, aspect=W / H), a.frames, W, H))
        # the path past the bin capacity (a first call whose pairs outgrow the initial size): bins for half of the default camera's pairs
        half = out[0]["bin_entries"] // 2
        ren.debug_raster_bin_capacity(half)
        out.append(case(ren, f"renderRaster scene, default camera, bins for {half} of {out[0]['bin_entries']} pairs (fallback walk)", draws,
                        scenes.camera("default", aspect=W / H), max(a.frames // 5, 3), W, H))
        ren.debug_raster_bin_capacity(0)
        pos, idx = meshgen.million_triangle_scene()[:2]
        ren.raster_mesh(3, pos, idx)
        out.append(case(ren, "1M-triangle scene, identity model", [rt.raster_draw(3, None, (0.8, 0.7, 0.6))], scenes.camera("default", aspect=W / H),
                        a.frames, W, H))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
