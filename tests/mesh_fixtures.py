"""Meshes, poses, random attributes and the host side of a dressed frame, shared by the CPU and the GPU tests of the dynamic mesh's shading extensions
(DESIGN.md 14.12-14.15).  Nothing here needs a GPU: positions come from the host definitions (skin_positions, gather_triangles), trees from
bvh_build_ref.ref_build -- the definition of the device's builder, ties included -- and refit_bvh, and the rows of a dress from the numpy
restatements tests/*_ref.py."""
import functools

import numpy as np

import colors_ref
import normals_ref
import opengl_raytracing_amd as rt
import scenes
import uvs_ref
from bvh_build_ref import ref_build
from test_mesh_normals_host import flat_grid

f32 = np.float32
IDENT = np.eye(4, dtype=f32).reshape(-1)
W, H = 64, 48
GREY = f32(0.85)
COORDS = [0, 1, 2, 4, 5, 6, 8, 9, 10]      # the nine geometry floats of a 12-float row


def two_bone_skin(v):
    """Two bones blended along x: (bone_idx [V,4], weights [V,4])."""
    x = v[:, 0]
    span = max(float(x.max() - x.min()), 1e-6)
    t = np.clip((x - x.min()) / f32(span) * f32(2.0) - f32(0.5), 0, 1).astype(f32)
    w = np.zeros((v.shape[0], 4), f32)
    w[:, 0], w[:, 1] = f32(1.0) - t, t
    bi = np.zeros((v.shape[0], 4), np.uint16)
    bi[:, 1] = 1
    return bi, w


@functools.lru_cache(maxsize=None)
def sphere():
    """The 1 280-triangle icosphere with two bones blended along x, read only."""
    v, f = rt.meshgen.icosphere(3)
    v = np.ascontiguousarray(v, f32)
    f = np.ascontiguousarray(f, np.uint32).reshape(-1)
    bi, w = two_bone_skin(v)
    for a in (v, f, bi, w):
        a.setflags(write=False)
    return v, f, bi, w


@functools.lru_cache(maxsize=None)
def flat():
    """The flat anchor: a floor at y = 1 facing up and, two units above it, a ceiling facing down, both grids of unit right triangles at integer
    coordinates in front of the close-up camera -> (positions, indices), read only.  Bounce and AO rays from one meet the other."""
    nx, nz = 6, 5
    v, f = flat_grid(nx, nz)
    floor = (v + np.array([-5, 1, -4], f32)).astype(f32)
    ceiling = (v + np.array([-5, 3, -4], f32)).astype(f32)
    at = lambda i, j: v.shape[0] + i * (nz + 1) + j      # noqa: E731
    f2 = []                                                                     # e1 = (0, 0, +-1), e2 = (-+1, 0, 0): cross(e1, e2) = (+0, -1, +0) exactly
    for i in range(nx):
        for j in range(nz):
            f2 += [at(i + 1, j), at(i + 1, j + 1), at(i, j), at(i, j + 1), at(i, j), at(i + 1, j + 1)]
    v, f = np.concatenate([floor, ceiling]), np.concatenate([f, np.array(f2, np.uint32)]).astype(np.uint32)
    for a in (v, f):
        a.setflags(write=False)
    return v, f


def turn(k):
    """A model matrix that turns the mesh about an oblique axis and stretches it: the medians of the next rebuild fall elsewhere."""
    a = 0.9 * k
    c, s = np.cos(a), np.sin(a)
    M = np.eye(4)
    M[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, c, -s], [0, s, c]]) @ np.diag([1.0 + 0.3 * abs(k), 1.0, 1.0 / (1.0 + 0.2 * abs(k))])
    M[:3, 3] = [0.2 * k, -0.1 * k, 0.05]
    return np.ascontiguousarray(M.T, f32).reshape(-1)


def bones(k):
    """Step k of the bend: bone 1 turned about z by 0.12 rad per step -- its end of the mesh moves by a few pixels of a 64 x 48 frame."""
    a = 0.12 * k
    M = np.eye(4)
    M[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    return np.stack([IDENT, np.ascontiguousarray(M.T, f32).reshape(-1)]).astype(f32)


def placed_turned():
    """The default placement turned about y and stretched: column-major, as the library takes it."""
    c, s = np.cos(0.6), np.sin(0.6)
    M = np.eye(4)
    M[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.diag([0.55, 0.5, 0.45])
    M[:3, 3] = [-2.0, 1.5, 0.0]
    return np.ascontiguousarray(M.T, f32).reshape(-1)


def random_colors(nv, seed):
    return np.random.default_rng(seed).uniform(0.05, 1.0, (nv, 3)).astype(f32)


def random_uvs(nv, seed):
    return np.random.default_rng(seed).uniform(-1.5, 2.5, (nv, 2)).astype(f32)


def random_texture(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4)).astype(np.uint8)


def uniforms(spp, frame, n, moved=True, use_bvh=True, gi=1, ao=1, taa=1):
    """A W x H frame of the close-up camera over a mesh of n triangles.  moved: the previous view-projection is that of a camera a step to the side, so
    the reference's own motion is non-zero and the resolve reprojects; else a static camera."""
    p, cam = rt.default_render_params(), scenes.camera("closeup", aspect=W / H)
    p.sppPerFrame, p.enableGI, p.enableAO, p.enableTAA = spp, gi, ao, taa
    L = rt.bvh_layout(n)
    prev = None
    if moved:
        before = scenes.camera("closeup", aspect=W / H)
        before.pos[2] += 0.07
        before.yaw -= 0.8
        prev = rt.mat4_mul(rt.camera_proj(before), rt.camera_view(before))
    u = rt.frame_uniforms(p, cam, W, H, frame, use_bvh, L.nNodes, L.nTris, prev_vp=prev)
    assert u.cameraMoved == int(moved) and u.enableGI == gi and u.enableAO == ao
    return u


# ---------------------------------------------------------------- the host side of the device's updates
class HostMesh:
    """What the device's scene is after each update, from the definitions alone: nodes12, tris12 and order (row -> input triangle) as ref_build gives
    them for a rebuild -- rt.build_bvh_order breaks equal medians its own way, the device's builders follow ref_build's tie rule -- and refit_bvh for
    a refit, and prev_tris, the previous pose's rows carried into the current row order (the current rows after the
    first rebuild)."""

    def __init__(self, indices):
        self.f = np.ascontiguousarray(indices, np.uint32).reshape(-1)
        self.nodes = self.tris = self.order = self.prev_tris = None

    def _carry(self, tris, order):
        if self.tris is None:
            return tris.copy()
        row_of = np.empty(order.size, np.int64)
        row_of[self.order] = np.arange(order.size)          # old row of every input triangle
        return self.tris[row_of[order]]

    def rebuild(self, tris9):
        nodes, tris, order = ref_build(tris9)
        self.prev_tris = self._carry(tris, order)
        self.nodes, self.tris, self.order = nodes, tris, np.ascontiguousarray(order, np.int32)
        return self

    def refit(self, tris9):
        nodes, tris = rt.refit_bvh(self.nodes, self.tris, self.order, tris9)
        self.prev_tris = self._carry(tris, self.order)
        self.nodes, self.tris = nodes, tris
        return self


def normal_rows(tris12, order, indices, n_verts):
    """[T,12]: the three corner normals (x, y, z, 0) of every row, from normals_ref.vertex_normals."""
    vn = normals_ref.vertex_normals(tris12, order, indices, n_verts)
    ix = np.asarray(indices, np.int64).reshape(-1, 3)[np.asarray(order, np.int64)]
    out = np.zeros((ix.shape[0], 3, 4), f32)
    out[:, :, :3] = vn[ix]
    return out.reshape(-1, 12), vn


def table(flags):
    """The 256 decoded values of a texture with these flags: the library's sRGB table, or c / 255."""
    return rt.srgb_table() if flags & uvs_ref.SRGB else (np.arange(256, dtype=f32) / f32(255)).astype(f32)


def dress(host, n_verts, normals=False, colors=None, uvs=None, texels=None, flags=0, motion=False):
    """The oracle's dress (a dict for oracle.render / oracle.dress_hits) of a HostMesh from the numpy definitions."""
    d = {}
    if normals:
        d["nrm_rows"] = normal_rows(host.tris, host.order, host.f, n_verts)[0]
    if colors is not None:
        d["col_rows"] = colors_ref.color_rows(host.order, host.f, colors)
    if uvs is not None:
        d["uv_rows"] = uvs_ref.uv_rows(host.order, host.f, uvs)
    if texels is not None:
        d.update(texels=np.ascontiguousarray(texels, np.uint8), flags=int(flags), table=table(flags))
    if motion:
        d["prev_tris"] = host.prev_tris
    return d


def same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


# ---------------------------------------------------------------- the three-part mesh
PART_FIRST = np.array([0, 100, 220, 300], np.int32)


@functools.lru_cache(maxsize=None)
def parts_mesh():
    """300 random triangles over shared vertices, split 100 / 120 / 80 into three parts -> (positions, indices), read only."""
    n = 300
    rng = np.random.default_rng(n)
    nv = n // 2 + 3
    v = rng.normal(0, 1, (nv, 3)).astype(f32)
    f = rng.integers(0, nv, (n, 3)).astype(np.uint32).reshape(-1)
    for a in (v, f):
        a.setflags(write=False)
    return v, f


def part_models(k):
    """Step k of the three parts' model matrices [3,16]: the default placement, each part turned its own way and shrunk so that all three -- and the
    sky around them -- are in the close-up camera's view."""
    D = np.asarray(rt.default_bvh_transform(), np.float64).reshape(4, 4).T
    S = np.diag([0.4, 0.4, 0.4, 1.0])
    out = []
    for p in range(3):
        T = np.asarray(turn(0.3 * (p - 1) + 0.2 * k), np.float64).reshape(4, 4).T
        out.append(np.ascontiguousarray((D @ T @ S).T, f32).reshape(-1))
    return np.stack(out)
