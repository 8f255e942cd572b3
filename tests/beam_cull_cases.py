"""Shared cases of the beam-cull tests (test_beam_cull_host.py, test_gpu_beam_cull.py; DESIGN.md 4.2 "Beam cull"): the views, their uniform blocks, and the
float32 restatement of slab() (rt_device_shade.hpp:128) the host tests hold rt_beam.hpp against."""
import functools

import numpy as np

import opengl_raytracing_amd as rt
import scenes
import test_gpu_queue_diet as qd

f32 = np.float32
K = 8      # sub-frames of a case's launch set

# name -> (mesh, W, H, camera position or None = the stock close-up, yaw)
CASES = {
    "bunny2_64x48": ("bunny2", 64, 48, None, -90.0),
    "bunny2_160x96": ("bunny2", 160, 96, None, -90.0),
    "bunny3_64x48": ("bunny3", 64, 48, None, -90.0),
    "bunny3_160x96": ("bunny3", 160, 96, None, -90.0),          # the non-vacuity case: dead tiles, and kept tiles that hold a missing pixel
    "two_mesh_160x96": ("two_mesh", 160, 96, None, -90.0),
    "one_leaf_64x48": ("one_leaf", 64, 48, (0.25, 0.9, 3.0), -90.0),
    "inside_root_box_64x48": ("bunny3", 64, 48, (-2.01, 1.51, 0.01), -90.0),
    "misses_root_box_64x48": ("bunny3", 64, 48, None, 90.0),     # the close-up camera turned round and up (no axis changes sign in a tile): no ray meets the root box
}


@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == "two_mesh":
        return qd._mesh("two_mesh")
    if name == "one_leaf":
        return scenes.one_leaf_mesh()
    return scenes.bunny_bvh(int(name[-1]))


@functools.lru_cache(maxsize=None)
def packed(name):
    return rt.pack_scene(*mesh(name))


def camera(case):
    _, w, h, pos, yaw = CASES[case]
    cam = scenes.camera("closeup", aspect=w / h)
    if pos is not None:
        cam.pos[0], cam.pos[1], cam.pos[2] = pos
    cam.yaw = yaw
    if yaw > 0:
        cam.pitch = 40.0
    return cam


def uniforms(case, frames=K, params=(("sppPerFrame", 2),)):
    m, w, h, _, _ = CASES[case]
    nodes, tris = mesh(m)
    p = rt.default_render_params()
    for k, v in params:
        setattr(p, k, v)
    cam = camera(case)
    return [rt.frame_uniforms(p, cam, w, h, f, True, nodes.shape[0], tris.shape[0]) for f in range(frames)]


def jitters(us):
    return np.array([[u.jitter[0], u.jitter[1]] for u in us], f32)


@functools.lru_cache(maxsize=None)
def host_cull(case, rank=0, world=1, frames=K):
    """(dead, stats, rd_inv [K, H, W, 3]) of the case by the host definition."""
    m = CASES[case][0]
    us = uniforms(case, frames)
    return rt.beam_cull(us[0], *mesh(m), jitters=jitters(us), rank=rank, world=world, rays=True, packed=packed(m))


def tile_of_pixels(w, h):
    """[H, W] -> index of the pixel's 16x16 tile (one rank: local tile == tile)."""
    tx = (w + 15) // 16
    y, x = np.mgrid[0:h, 0:w]
    return (y // 16) * tx + x // 16


def slab(ro, rd_inv, lo, hi):
    """slab() in float32 numpy, operation for operation -> (tmax >= tmin, tmin, tmax); arrays broadcast over the last axis of 3."""
    ro, rd_inv, lo, hi = (np.asarray(a, f32) for a in (ro, rd_inv, lo, hi))
    with np.errstate(all="ignore"):
        t0 = ((lo - ro).astype(f32) * rd_inv).astype(f32)
        t1 = ((hi - ro).astype(f32) * rd_inv).astype(f32)
        n, f = np.fmin(t0, t1), np.fmax(t0, t1)
        tmin = np.fmax(np.fmax(n[..., 0], n[..., 1]), np.fmax(n[..., 2], f32(0.0)))
        tmax = np.fmin(np.fmin(f[..., 0], f[..., 1]), f[..., 2])
        return tmax >= tmin, tmin, tmax
