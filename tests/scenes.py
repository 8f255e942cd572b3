"""Shared scene builders for tests and bench (inputs only; no rendering here)."""
from __future__ import annotations

import functools
from pathlib import Path

import numpy as np

import opengl_raytracing_amd as rt

ROOT = Path(__file__).resolve().parent.parent
ASSETS = ROOT / "assets" / "cubemaps"


@functools.lru_cache(maxsize=8)
def env_faces(name="Sky_01"):
    return rt.load_cubemap_cross(ASSETS / f"{name}.png")


@functools.lru_cache(maxsize=8)
def bunny_bvh(subdiv=6):
    """(nodes12, tris12) of the procedural bunny stand-in under defaultBvhTransform, built by the PRODUCT host code."""
    v, f = rt.meshgen.bunny_standin(subdiv)
    tris9 = rt.gather_triangles(v, f)
    return rt.build_bvh(tris9)


@functools.lru_cache(maxsize=1)
def million_bvh():
    """(nodes12, tris12) of BASELINE configs[4]'s 1 M-triangle scene (meshgen.million_triangle_scene, identity model), built by the PRODUCT host code."""
    v, f = rt.meshgen.million_triangle_scene()
    return rt.build_bvh(rt.gather_triangles(v, f, np.eye(4, dtype=np.float32).reshape(-1)))


def reference_window_inputs(mesh, env):
    """(nodes12, tris12, faces) named by a windowed reference fixture (tests/golden/glsl_k_*.npz): mesh "bench" (bunny_bvh(6), the bench
    mesh), "million" (million_bvh()) or "" (analytic scene); env a cube map under assets/cubemaps or "" (gradient sky)."""
    nodes, tris = {"bench": bunny_bvh, "million": million_bvh}[mesh]() if mesh else (None, None)
    return nodes, tris, env_faces(env) if env else None


def tiny_env(n=8, seed=3):
    """Small random RGB cube map (exercises face seams and bilinear weights)."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, size=(6, n, n, 3), dtype=np.uint8)


def camera(kind="default", aspect=None):
    c = rt.default_camera() if kind == "default" else rt.closeup_camera()
    if aspect is not None:
        c.aspect = aspect
    return c


def one_leaf_mesh():
    """Two triangles: a BVH of a single leaf (no inner node, no quantised tree)."""
    tris9 = np.array([[-1, 0, -1, 1, 0, -1, 0, 1.5, -1.2], [-1, 0, 1, 1, 0, 1, 0, 1.5, 0.5]], np.float32) + np.float32(0.25)
    return rt.build_bvh(tris9)


def adversarial_rays(nodes, tris, n=6000, seed=11):
    """(origins, dirs, tmax) of 7 n rays where traversal kernels go wrong, for the ray-by-ray tests of the production traversal kernels:
    random rays towards the mesh; axis-parallel rays (1/0 = inf slabs) whose origin coordinates sit EXACTLY on planes of node boxes; rays that
    start on triangle vertices and edge midpoints (what shadow and AO rays do); rays aimed at box corners; rays with denormal-size or -0.0
    direction components.  tmax: 0.05 - 3 times the root box's largest extent."""
    rng = np.random.default_rng(seed)
    lo, hi = nodes[:, 0:3], nodes[:, 4:7]
    centre = ((lo[0] + hi[0]) * 0.5).astype(np.float32)
    ext = float((hi[0] - lo[0]).max())
    f32 = np.float32

    def unit(v):
        v = v.astype(np.float32)
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)

    O, D = [], []
    # (1) random rays towards the mesh
    o = (centre + rng.normal(size=(n, 3)) * ext).astype(f32)
    O.append(o); D.append(unit(centre + rng.uniform(-0.4, 0.4, (n, 3)) * ext - o))
    # (2) axis-parallel rays lying exactly in planes of node boxes (two coordinates of the origin taken from box corners of random nodes)
    for axis in range(3):
        k = rng.integers(0, nodes.shape[0], n)
        corner = np.where(rng.random((n, 3)) < 0.5, lo[k], hi[k]).astype(f32)
        o = corner.copy()
        o[:, axis] = (centre[axis] + np.where(rng.random(n) < 0.5, -1.0, 1.0) * ext * 1.5).astype(f32)
        d = np.zeros((n, 3), f32)
        d[:, axis] = -np.sign(o[:, axis] - centre[axis])
        O.append(o); D.append(d)
    # (3) rays leaving triangle vertices and edge midpoints
    k = rng.integers(0, tris.shape[0], n)
    v0, e1, e2 = tris[k, 0:3], tris[k, 4:7], tris[k, 8:11]
    start = np.where((rng.random(n) < 0.5)[:, None], v0, (v0 + f32(0.5) * e1).astype(f32)).astype(f32)
    O.append(start); D.append(unit(rng.normal(size=(n, 3))))
    # (4) rays aimed exactly at corners of node boxes
    k = rng.integers(0, nodes.shape[0], n)
    corner = np.where(rng.random((n, 3)) < 0.5, lo[k], hi[k]).astype(f32)
    o = (centre + unit(rng.normal(size=(n, 3))) * ext * 2.0).astype(f32)
    O.append(o); D.append(unit(corner - o))
    # (5) direction components of denormal size and exact zeros mixed in
    o = (centre + rng.normal(size=(n, 3)) * ext).astype(f32)
    d = unit(centre - o)
    tiny = rng.integers(0, 3, n)
    d[np.arange(n), tiny] = np.where(rng.random(n) < 0.5, f32(1e-41), f32(-0.0))
    O.append(o); D.append(d)
    org, dirs = np.concatenate(O).astype(f32), np.concatenate(D).astype(f32)
    tmax = rng.uniform(0.05, 3.0, org.shape[0]).astype(f32) * f32(ext)
    return org, dirs, tmax
