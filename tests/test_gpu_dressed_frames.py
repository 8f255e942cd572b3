"""Frames of the dressed dynamic mesh against the dressed CPU oracle (oracle/orc_dress.h): smooth normals (14.13), colours (14.14), UVs
with an albedo texture (14.15) and object motion (14.12), alone and together, on both pipelines, bit for bit on all four targets.

The oracle's inputs are built on the host from the definitions, never from device read-backs: positions by skin_positions, the tree and its rows by
gather_triangles -> bvh_build_ref.ref_build (a rebuild: the numpy definition of the device's builder, whose rule for equal medians the host's
build_bvh_order does not share) or refit_bvh (a refit), the rows of the dress by the numpy restatements tests/*_ref.py, the previous
pose by carrying the rows of the update before into the current order (mesh_fixtures.HostMesh).  One assertion per case holds the device's
mesh_order() to the host's, so that a tree mismatch reports itself as one."""
import functools

import numpy as np
import pytest

import colors_ref
import mesh_fixtures as mf
import opengl_raytracing_amd as rt
import oracle as orc
import scenes
import uvs_ref
from mesh_fixtures import GREY, H, IDENT, W, same

pytestmark = pytest.mark.gpu

f32 = np.float32
TARGETS = ("color", "motion", "gpos", "gnrm")
PIPELINES = [rt.RT_PIPELINE_WAVEFRONT, rt.RT_PIPELINE_MEGAKERNEL]
KINDS = ("normals", "colors", "uvs", "uvs-nearest-1x1", "motion")
SPPS = (1, 2)


def _faces():
    return scenes.tiny_env(8)


def _attributes(kind, nv):
    """What a case of the skinned sphere wears -> dict(normals, colors, uvs, texels, flags, motion)."""
    a = dict(normals=False, colors=None, uvs=None, texels=None, flags=0, motion=False)
    if kind in ("normals", "all"):
        a["normals"] = True
    if kind in ("colors", "all"):
        a["colors"] = mf.random_colors(nv, 6)
    if kind in ("uvs", "all"):
        a.update(uvs=mf.random_uvs(nv, 12), texels=mf.random_texture(3, 5, 13), flags=(uvs_ref.SRGB | uvs_ref.CLAMP) if kind == "all" else 0)
    if kind == "uvs-nearest-1x1":
        a.update(uvs=mf.random_uvs(nv, 12), texels=np.array([[[200, 90, 30, 77]]], np.uint8), flags=uvs_ref.NEAREST)
    if kind in ("motion", "all"):
        a["motion"] = True
    return a


def _wear(b, a):
    """The attributes on a context whose mesh is uploaded and has no tree yet."""
    if a["colors"] is not None:
        b.mesh_colors_enable()
        b.mesh_set_colors(a["colors"])
    if a["normals"]:
        b.mesh_normals_enable()
    if a["motion"]:
        b.mesh_motion_enable()
    if a["uvs"] is not None:
        b.mesh_uvs_enable()
        b.mesh_set_uvs(a["uvs"])
        b.mesh_texture_upload(a["texels"], a["flags"])


def _sphere_context(pipeline, a):
    v, f, bi, w = mf.sphere()
    b = rt.Renderer(pipeline=pipeline)
    b.upload_env(_faces())
    b.resize(W, H)
    b.mesh_upload(v, f)
    b.mesh_skin_upload(bi, w, 2, rest=v)
    _wear(b, a)
    b.mesh_rebuild(rt.default_bvh_transform())
    return b


def _skin_step(b, k):
    b.mesh_set_bones(mf.bones(k))
    b.mesh_skin()


def _check(got, want, what):
    """All four targets bit for bit; on a difference, the count of differing pixels per target."""
    bad = {name: int((g != w_).reshape(H * W, -1).any(axis=1).sum()) for name, g, w_ in zip(TARGETS, got, want) if not same(g, w_)}
    assert not bad, (what, bad)


def _hits_and_misses(host, u):
    rec, _ = orc.primary_hits(u, host.nodes, host.tris)
    hit = colors_ref.prims(rec) >= 0
    assert hit.sum() >= 200 and (~hit).sum() >= 200, (int(hit.sum()), int((~hit).sum()))


# ---------------------------------------------------------------- the host side of the sphere's chain, once
@functools.lru_cache(maxsize=None)
def _sphere_hosts():
    """The skinned sphere through the chain: at rest, after skin step 2 and a refit, after skin step 3 and a rebuild under placed_turned()
    -> three read-only HostMesh snapshots (nodes, tris, order, prev_tris)."""
    v, f, bi, w = mf.sphere()
    M = rt.default_bvh_transform()
    host = mf.HostMesh(f).rebuild(rt.gather_triangles(v, f, M))
    out = [_snapshot(host)]
    host.refit(rt.gather_triangles(rt.skin_positions(v, bi, w, mf.bones(2)), f, M))
    out.append(_snapshot(host))
    host.rebuild(rt.gather_triangles(rt.skin_positions(v, bi, w, mf.bones(3)), f, mf.placed_turned()))
    out.append(_snapshot(host))
    return tuple(out)


def _snapshot(host):
    s = mf.HostMesh(host.f)
    s.nodes, s.tris, s.order, s.prev_tris = host.nodes.copy(), host.tris.copy(), host.order.copy(), host.prev_tris.copy()
    for a in (s.nodes, s.tris, s.order, s.prev_tris):
        a.setflags(write=False)
    return s


# ---------------------------------------------------------------- 1: each extension alone
@functools.lru_cache(maxsize=None)
def _alone_device(pipeline, kind):
    """One context per (pipeline, kind): the sphere after a skin step and a refit -> {spp: targets}, and the device's order."""
    nv, n = mf.sphere()[0].shape[0], mf.sphere()[1].size // 3
    out = {}
    with _sphere_context(pipeline, _attributes(kind, nv)) as b:
        _skin_step(b, 2)
        b.mesh_refit(rt.default_bvh_transform())
        out["order"] = b.mesh_order(as_torch=False).copy()
        for spp in SPPS:
            b.reset_accum()
            b.render_frame(mf.uniforms(spp, 0, n))
            out[spp] = b.read_all()
    return out


@functools.lru_cache(maxsize=None)
def _alone_oracle(kind, spp):
    nv, n = mf.sphere()[0].shape[0], mf.sphere()[1].size // 3
    host = _sphere_hosts()[1]
    u = mf.uniforms(spp, 0, n)
    _hits_and_misses(host, u)
    d = mf.dress(host, nv, **_attributes(kind, nv))
    want, _ = orc.render(u, host.nodes, host.tris, _faces(), dress=d)
    plain, _ = orc.render(u, host.nodes, host.tris, _faces())
    return want, plain


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_each_extension_alone(pipeline, kind, spp):
    got = _alone_device(pipeline, kind)
    assert np.array_equal(got["order"], _sphere_hosts()[1].order), "the device's tree is not the host's"
    want, plain = _alone_oracle(kind, spp)
    assert mf.uniforms(spp, 0, 1280).cameraMoved == 1
    moves = {"normals": 0, "colors": 0, "uvs": 0, "uvs-nearest-1x1": 0, "motion": 1}[kind]
    assert not same(want[moves], plain[moves]), "the dress does nothing in this case"
    _check(got[spp], want, (kind, spp))


# ---------------------------------------------------------------- 2: everything together, three frames with history
@functools.lru_cache(maxsize=None)
def _chain_device(pipeline, spp):
    nv, n = mf.sphere()[0].shape[0], mf.sphere()[1].size // 3
    frames, orders = [], []
    with _sphere_context(pipeline, _attributes("all", nv)) as b:
        b.reset_accum()
        for k in range(3):
            if k == 1:
                _skin_step(b, 2)
                b.mesh_refit(rt.default_bvh_transform())
            if k == 2:
                _skin_step(b, 3)
                b.mesh_rebuild(mf.placed_turned())
            orders.append(b.mesh_order(as_torch=False).copy())
            b.render_frame(mf.uniforms(spp, k, n))
            frames.append(b.read_all())
    return frames, orders


@functools.lru_cache(maxsize=None)
def _chain_oracle(spp):
    nv, n = mf.sphere()[0].shape[0], mf.sphere()[1].size // 3
    a = _attributes("all", nv)
    frames, prev = [], None
    for k, host in enumerate(_sphere_hosts()):
        u = mf.uniforms(spp, k, n)
        _hits_and_misses(host, u)
        want, _ = orc.render(u, host.nodes, host.tris, _faces(), prev, dress=mf.dress(host, nv, **a))
        frames.append(want)
        prev = want[0]                                              # each frame's history is the oracle's own previous COLOR0
    return frames


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_everything_together_over_three_frames(pipeline, spp):
    frames, orders = _chain_device(pipeline, spp)
    hosts = _sphere_hosts()
    assert not np.array_equal(hosts[2].order, hosts[1].order), "the rebuild kept every triangle in its row: the case does not reorder"
    assert not same(hosts[1].prev_tris, hosts[1].tris) and not same(hosts[2].prev_tris, hosts[2].tris)
    for k in range(3):
        assert np.array_equal(orders[k], hosts[k].order), (k, "the device's tree is not the host's")
    want = _chain_oracle(spp)
    for k in range(3):
        _check(frames[k], want[k], ("frame", k, spp))
    assert not same(want[1][0], want[2][0])


# ---------------------------------------------------------------- 3: colour bleeding with a reference
@functools.lru_cache(maxsize=None)
def _flat_host():
    v, f = mf.flat()
    return mf.HostMesh(f).rebuild(rt.gather_triangles(v, f, IDENT))


def _red_ceiling():
    nv = mf.flat()[0].shape[0]
    colors = np.full((nv, 3), GREY, f32)
    colors[nv // 2:] = [GREY, 0, 0]                                 # the ceiling's vertices
    return colors


@functools.lru_cache(maxsize=None)
def _bleeding_oracle(spp):
    host, nv, n = _flat_host(), mf.flat()[0].shape[0], mf.flat()[1].size // 3
    u = mf.uniforms(spp, 0, n)
    _hits_and_misses(host, u)
    want, _ = orc.render(u, host.nodes, host.tris, _faces(), dress=mf.dress(host, nv, colors=_red_ceiling()))
    plain, _ = orc.render(u, host.nodes, host.tris, _faces())
    return want, plain


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_a_red_ceiling_bleeds_as_the_oracle_says(pipeline, spp):
    v, f = mf.flat()
    n = f.size // 3
    host = _flat_host()
    with rt.Renderer(pipeline=pipeline) as b:
        b.upload_env(_faces())
        b.resize(W, H)
        b.mesh_upload(v, f)
        b.mesh_colors_enable()
        b.mesh_set_colors(_red_ceiling())
        b.mesh_rebuild(IDENT)
        assert np.array_equal(b.mesh_order(as_torch=False), host.order), "the device's tree is not the host's"
        b.reset_accum()
        b.render_frame(mf.uniforms(spp, 0, n))
        got = b.read_all()
    want, plain = _bleeding_oracle(spp)
    # the premise, on the oracle: the grey floor (rows at y = 1) loses green where the red ceiling is above it
    rec, _ = orc.primary_hits(mf.uniforms(spp, 0, n), host.nodes, host.tris)
    prim = colors_ref.prims(rec)
    floor = ((prim >= 0) & (host.tris[np.where(prim >= 0, prim, 0), 1] == 1)).reshape(H, W)
    g_on, g_off = orc.half_to_float(want[0])[..., 1], orc.half_to_float(plain[0])[..., 1]
    assert floor.sum() >= 100 and (g_on[floor] < g_off[floor]).sum() >= 50
    _check(got, want, ("red ceiling", spp))


# ---------------------------------------------------------------- 4: parts
@functools.lru_cache(maxsize=None)
def _parts_oracle(spp):
    v, f = mf.parts_mesh()
    nv, n = v.shape[0], f.size // 3
    host = mf.HostMesh(f).rebuild(rt.gather_triangles_parts(v, f, mf.PART_FIRST, mf.part_models(0)))
    host.refit(rt.gather_triangles_parts(v, f, mf.PART_FIRST, mf.part_models(1)))
    colors = colors_ref.vertex_colors_from_parts(f, mf.PART_FIRST, _part_rgb(), nv)
    u = mf.uniforms(spp, 0, n)
    _hits_and_misses(host, u)
    d = mf.dress(host, nv, normals=True, colors=colors, motion=True)
    want, _ = orc.render(u, host.nodes, host.tris, _faces(), dress=d)
    return want, host.order


def _part_rgb():
    return np.array([[0.9, 0.2, 0.1], [0.15, 0.8, 0.3], [0.2, 0.25, 0.95]], f32)


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_parts(pipeline, spp):
    v, f = mf.parts_mesh()
    nv, n = v.shape[0], f.size // 3
    want, order = _parts_oracle(spp)
    with rt.Renderer(pipeline=pipeline) as b:
        b.upload_env(_faces())
        b.resize(W, H)
        b.mesh_upload_parts(v, f, mf.PART_FIRST)
        b.mesh_colors_enable()
        b.mesh_set_colors(rt.vertex_colors_from_parts(f, mf.PART_FIRST, _part_rgb(), nv))
        b.mesh_normals_enable()
        b.mesh_motion_enable()
        b.mesh_set_part_matrices(mf.part_models(0))
        b.mesh_rebuild_parts()
        b.mesh_set_part_matrices(mf.part_models(1))
        b.mesh_refit_parts()
        assert np.array_equal(b.mesh_order(as_torch=False), order), "the device's tree is not the host's"
        b.reset_accum()
        b.render_frame(mf.uniforms(spp, 0, n))
        got = b.read_all()
    _check(got, want, ("parts", spp))


# ---------------------------------------------------------------- 4b: bounce and AO rays that meet the dressed mesh
# The sphere is convex and the floor and ceiling are flat: on the first hardly a bounce or AO ray meets the mesh again, on the second every attribute
# that varies over a triangle is missing.  The 300 random triangles as ONE mesh wear everything at once, so that the bounce hit's normal, colour and
# texel are taken at barycentrics of their own on triangles that differ from the primary hit's, and AO rays are stopped according to the normal.
@functools.lru_cache(maxsize=None)
def _soup_case(spp):
    v, f = mf.parts_mesh()
    nv, n = v.shape[0], f.size // 3
    a = dict(normals=True, colors=mf.random_colors(nv, 21), uvs=mf.random_uvs(nv, 22), texels=mf.random_texture(3, 5, 23), flags=0, motion=True)
    host = mf.HostMesh(f).rebuild(rt.gather_triangles(v, f, mf.part_models(0)[1]))
    host.refit(rt.gather_triangles(v, f, mf.part_models(1)[1]))
    u = mf.uniforms(spp, 0, n)
    _hits_and_misses(host, u)
    want, cnt = orc.render(u, host.nodes, host.tris, _faces(), dress=mf.dress(host, nv, **a))
    # the premise, on the oracle: bounce rays hit the mesh (only a bounce HIT casts shadow rays of its own) and AO rays are stopped
    _, no_gi = orc.render(mf.uniforms(spp, 0, n, gi=0), host.nodes, host.tris, _faces())
    plain_frame, plain = orc.render(u, host.nodes, host.tris, _faces())
    assert plain.raysShadow - no_gi.raysShadow >= 4 * 200 * spp, (plain.raysShadow, no_gi.raysShadow)
    ao_off, _ = orc.render(mf.uniforms(spp, 0, n, ao=0), host.nodes, host.tris, _faces())
    assert (ao_off[0] != plain_frame[0]).any(axis=2).sum() >= 200
    return a, want, host.order


@pytest.mark.parametrize("spp", SPPS)
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_bounce_and_ao_rays_meet_the_dressed_mesh(pipeline, spp):
    v, f = mf.parts_mesh()
    n = f.size // 3
    a, want, order = _soup_case(spp)
    with rt.Renderer(pipeline=pipeline) as b:
        b.upload_env(_faces())
        b.resize(W, H)
        b.mesh_upload(v, f)
        _wear(b, a)
        b.mesh_rebuild(mf.part_models(0)[1])
        b.mesh_refit(mf.part_models(1)[1])
        assert np.array_equal(b.mesh_order(as_torch=False), order), "the device's tree is not the host's"
        b.reset_accum()
        b.render_frame(mf.uniforms(spp, 0, n))
        got = b.read_all()
    _check(got, want, ("soup", spp))


# ---------------------------------------------------------------- 5: a batch of static-camera frames
def test_a_batch_of_four_frames():
    nv, n = mf.sphere()[0].shape[0], mf.sphere()[1].size // 3
    a = _attributes("all", nv)
    host = _sphere_hosts()[1]
    us = [mf.uniforms(2, k, n, moved=False) for k in range(4)]
    with _sphere_context(rt.RT_PIPELINE_WAVEFRONT, a) as b:
        _skin_step(b, 2)
        b.mesh_refit(rt.default_bvh_transform())
        assert np.array_equal(b.mesh_order(as_torch=False), host.order), "the device's tree is not the host's"
        b.reset_accum()
        b.render_frames(us)
        got = b.read_all()
    d = mf.dress(host, nv, **a)
    prev = None
    for u in us:
        want, _ = orc.render(u, host.nodes, host.tris, _faces(), prev, dress=d)
        prev = want[0]
    _check(got, want, "batch")


# ---------------------------------------------------------------- 6: the hybrid scene against the undressed oracle
@pytest.mark.parametrize("pipeline", PIPELINES)
def test_hybrid_is_the_undressed_oracle(pipeline):
    nv, n = mf.sphere()[0].shape[0], mf.sphere()[1].size // 3
    host = _sphere_hosts()[1]
    u = mf.uniforms(2, 0, n, use_bvh=rt.RT_SCENE_HYBRID)
    with _sphere_context(pipeline, _attributes("all", nv)) as b:
        _skin_step(b, 2)
        b.mesh_refit(rt.default_bvh_transform())
        assert np.array_equal(b.mesh_order(as_torch=False), host.order), "the device's tree is not the host's"
        b.reset_accum()
        b.render_frame(u)
        got = b.read_all()
    want, cnt = orc.render(u, host.nodes, host.tris, _faces())
    assert cnt.hitPixels >= 200
    _check(got, want, "hybrid")
