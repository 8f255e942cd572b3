"""The dressed mode of the CPU oracle (oracle/orc_dress.h): smooth normals, colours, UVs with a texture and the previous pose of the
dynamic mesh in orc.render, pinned where it can be pinned without a GPU.  Off is off (the undressed frames are the ones recorded before the mode
existed); dress_hits equals the numpy definitions tests/{normals,colors,uvs,motion}_ref.py bit for bit, edge cases included; the identity dresses
render the undressed frame on all four targets; on the skinned icosphere GNRM and MOTION are f16 of the definitions at the oracle's own primary hits,
GPOS does not move and COLOR0 does; the hybrid scene ignores the dress.  Every comparison is exact."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import colors_ref
import mesh_fixtures as mf
import motion_ref
import normals_ref
import opengl_raytracing_amd as rt
import scenes
import uvs_ref
from mesh_fixtures import COORDS, GREY, H, IDENT, W, same

f32 = np.float32
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = Path(__file__).resolve().parent / "golden" / "oracle_undressed_64x48.npz"
TARGETS = ("color", "motion", "gpos", "gnrm")
INT_MAX = 2 ** 31 - 1
FOUR = np.float16(4.0).view(np.uint16)


def _half(a):
    return np.ascontiguousarray(a, f32).astype(np.float16).view(np.uint16)


# ---------------------------------------------------------------- scenes
@functools.lru_cache(maxsize=None)
def flat_scene():
    """The flat floor and ceiling under the identity: (HostMesh, n_verts, n_tris)."""
    v, f = mf.flat()
    return mf.HostMesh(f).rebuild(rt.gather_triangles(v, f, IDENT)), v.shape[0], f.size // 3


@functools.lru_cache(maxsize=None)
def sphere_scene():
    """The skinned icosphere after a rebuild at rest and a refit at bend step 2: (HostMesh, n_verts, n_tris, positions)."""
    v, f, bi, w = mf.sphere()
    M = rt.default_bvh_transform()
    host = mf.HostMesh(f).rebuild(rt.gather_triangles(v, f, M))
    pos = rt.skin_positions(v, bi, w, mf.bones(2))
    host.refit(rt.gather_triangles(pos, f, M))
    return host, v.shape[0], f.size // 3, pos


def undressed_frames(render):
    """The two frames of the off-is-off pin by render(u, nodes, tris, faces, prev) -> {name: array}: a BVH frame 1 over a frame 0 history and a
    hybrid frame of the flat scene, GI and AO on, spp 2, with their counters."""
    host, _, n = flat_scene()
    faces = scenes.tiny_env(8)
    out = {}
    first, _ = render(mf.uniforms(2, 0, n), host.nodes, host.tris, faces, None)
    for name, u in (("bvh", mf.uniforms(2, 1, n)), ("hybrid", mf.uniforms(2, 1, n, use_bvh=rt.RT_SCENE_HYBRID))):
        got, cnt = render(u, host.nodes, host.tris, faces, first[0])
        for t, a in zip(TARGETS, got):
            out[f"{name}/{t}"] = a
        out[f"{name}/counters"] = np.array(cnt.as_tuple(), np.uint64)
    return out


# ---------------------------------------------------------------- 1: off is off
def test_off_is_off(orc):
    want = np.load(GOLDEN)
    null = {}                                                                   # a dress whose pointers are all null
    plain = undressed_frames(lambda u, n, t, e, p: orc.render(u, n, t, e, p))
    nulled = undressed_frames(lambda u, n, t, e, p: orc.render(u, n, t, e, p, dress=null))
    assert sorted(want.files) == sorted(plain)
    for name in want.files:
        assert same(plain[name], want[name]), name
        assert same(nulled[name], want[name]), name
    assert (orc.half_to_float(want["bvh/color"])[..., :3] != 0).any() and want["bvh/counters"][6] >= 200      # hitPixels


def test_a_dress_does_not_outlive_its_render(orc):
    host, nv, n = flat_scene()
    faces = scenes.tiny_env(8)
    u = mf.uniforms(1, 0, n)
    before, _ = orc.render(u, host.nodes, host.tris, faces)
    red = np.tile(np.array([GREY, 0, 0], f32), (nv, 1))
    dressed, _ = orc.render(u, host.nodes, host.tris, faces, dress=mf.dress(host, nv, colors=red))
    assert not same(dressed[0], before[0])
    with pytest.raises(ValueError):                                             # rows for another mesh: refused before anything is set
        orc.render(u, host.nodes, host.tris, faces, dress={"col_rows": np.zeros((n + 1, 12), f32)})
    with pytest.raises(RuntimeError):                                           # refused by the render itself: cleared all the same
        orc.render(rt.RtUniforms(), host.nodes, host.tris, faces, dress=mf.dress(host, nv, colors=red))
    after, _ = orc.render(u, host.nodes, host.tris, faces)
    for name, x, y in zip(TARGETS, after, before):
        assert same(x, y), name
    out = np.full((4, 3), 7, f32)                                               # no dress: dress_hits' outputs stay as they are
    L = orc.lib()
    fp = lambda a: a.ctypes.data_as(orc._FP)      # noqa: E731
    assert L.orc_dress_hits(fp(host.tris), fp(np.zeros((4, 4), f32)), 4, fp(out), fp(out), fp(out)) == 4 and (out == 7).all()


# ---------------------------------------------------------------- 2: the per-hit rules
@functools.lru_cache(maxsize=None)
def _corner_case():
    """40 rows whose triangles own their three vertices (indices 0 .. 119, rows shuffled by `order`), so that every corner value can be chosen:
    tris12, order, indices, per-vertex normals / colours / UVs, previous rows -- the edge cases of the host tests in the first rows."""
    rng = np.random.default_rng(17)
    T = 40
    order = rng.permutation(T).astype(np.int32)
    f = np.arange(3 * T, dtype=np.uint32)
    tris = np.zeros((T, 12), f32)
    tris[:, COORDS] = rng.normal(0, 1, (T, 9)).astype(f32)
    tris[5, 8:11] = tris[5, 4:7]                                                # a degenerate row: its face normal is whatever 0 / 0 is
    nrm = rng.normal(0, 1, (3 * T, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
    col, uv = mf.random_colors(3 * T, 3), mf.random_uvs(3 * T, 4)
    corners = lambda row: 3 * order[row] + np.arange(3)      # noqa: E731
    nrm[corners(0)] = nrm[corners(0)[0]]                                        # bit-equal corners: n0 bit for bit
    nrm[corners(1)] = 0                                                         # bit-equal zeros: the face normal
    nrm[corners(2)[1]] = -nrm[corners(2)[0]]                                    # opposite corners: a zero blend at (0.5, 0)
    nrm[corners(3)[0]] = 0                                                      # one zero corner
    nrm[corners(4)] = [[0, 0, 1], [0, 0, 1], [-0.0, 0, 1]]                      # equal as numbers, not as bits: blended
    nrm[corners(6)] = [np.inf, 0, 0]                                            # bit-equal and not finite: handed back
    nrm[corners(7)[2]] = [np.nan, 0, 1]
    col[corners(0)] = col[corners(0)[0]]
    col[corners(1), 1] = col[corners(1)[0], 1]                                  # one flat channel
    col[corners(4), 0] = [0.0, 0.0, -0.0]
    uv[corners(0)] = uv[corners(0)[0]]
    uv[corners(1), 0] = uv[corners(1)[0], 0]
    uv[corners(6)[1]] = [np.nan, np.inf]                                        # non-finite UVs: sampled as 0
    prev = tris.copy()
    moved = np.arange(T) % 3 != 0                                               # every third row keeps its bits: the point's own bits
    prev[np.ix_(moved, COORDS)] += rng.normal(0, 0.05, (int(moved.sum()), 9)).astype(f32)
    tris[9, 0], prev[9, 0] = 0.0, -0.0                                          # +0 against -0: a changed row
    prev[12, 3], prev[12, 7] = 5, 6                                             # the padding floats are no geometry
    for a in (tris, order, f, nrm, col, uv, prev):
        a.setflags(write=False)
    return tris, order, f, nrm, col, uv, prev


def _records(n, seed=5):
    """n hit records on the 40 rows: the edge cases first (NaN, infinite and -0 barycentrics, prims off the mesh), then random hits."""
    T = 40
    rng = np.random.default_rng(seed)
    prim = rng.integers(0, T, 257).astype(np.int32)
    a = rng.uniform(0, 1, 257).astype(f32)
    b = (rng.uniform(0, 1, 257) * (1 - a)).astype(f32)
    a[::11], b[::13] = 0, 0
    prim[:24] = [2, 0, 1, 3, 4, 5, 6, 7, 9, 12, 0, 1, 2, 3, 8, 10, -1, T, INT_MAX, -INT_MAX - 1, 4, 9, 6, 7]
    a[:16] = [0.5, 0.3, 0.2, np.nan, np.inf, -np.inf, 0.25, -0.0, 0.1, 0.2, np.nan, 0.4, 1.0, 0.0, 1.5, -0.5]
    b[:16] = [0.0, 0.3, 0.5, 0.5, 0.25, 0.5, np.nan, 0.5, -0.0, 0.3, np.inf, np.nan, 0.0, 1.0, -0.75, 0.5]
    return colors_ref.records(prim, a, b)[:n].copy()


def _want_albedo(order, f, col, uv, tex, flags, rec):
    prim = colors_ref.prims(rec)
    on = (prim >= 0) & (prim < order.size)
    base = colors_ref.hit_colors(order, f, col, rec) if col is not None else np.where(on[:, None], GREY, f32(0)).astype(f32)
    if tex is None:
        return base
    texel = uvs_ref.sample_texture(tex, flags, uvs_ref.hit_uvs(order, f, uv, rec), mf.table(flags))
    with np.errstate(all="ignore"):
        return np.where(on[:, None], (base * texel).astype(f32), f32(0)).astype(f32)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_hit_rules_equal_the_numpy_definitions(orc, n):
    tris, order, f, nrm, col, uv, prev = _corner_case()
    rec = _records(n)
    pts = np.random.default_rng(n).normal(0, 2, (n, 3)).astype(f32)
    pts[0] = [-0.0, np.nan, 1.0]
    if n > 8:
        pts[8] = [-0.0, 1.0, 2.0]                                               # on row 9, whose only change is +0 against -0: x + (+0) is +0, not x's -0
    host = mf.HostMesh(f)
    host.tris, host.order, host.prev_tris = tris, order, prev
    ix = f.reshape(-1, 3)[order]
    nrows = np.zeros((40, 3, 4), f32)
    nrows[:, :, :3] = nrm[ix]
    d = mf.dress(host, 120, colors=col, uvs=uv, texels=mf.random_texture(3, 5, 8), flags=0, motion=True)
    d["nrm_rows"] = nrows.reshape(-1, 12)
    got_n, got_a, got_p = orc.dress_hits(d, tris, rec, pts)
    with np.errstate(all="ignore"):
        want_n = normals_ref.hit_normals(tris, order, f, nrm, rec)
    assert same(got_n, want_n), np.flatnonzero((got_n.view(np.uint32) != want_n.view(np.uint32)).any(axis=1))
    assert same(got_a, _want_albedo(order, f, col, uv, d["texels"], 0, rec))
    assert same(got_p, motion_ref.prev_points(tris, prev, rec, pts))
    if n >= 24:                                                                 # the premises of the edge cases, on the definitions themselves
        face = normals_ref.face_normals(tris)
        assert same(want_n[1], nrm[ix[0, 0]]) and same(want_n[2], face[1]) and same(want_n[0], face[2])      # bit-equal, zeros, a zero blend
        assert same(want_n[3], face[3]) and same(want_n[10], nrm[ix[0, 0]]) and same(want_n[11], face[1])    # NaN barycentrics
        assert (got_n[16:20].view(np.uint32) == 0).all() and (got_a[16:20].view(np.uint32) == 0).all() and (got_p[16:20].view(np.uint32) == 0).all()
        unchanged = (colors_ref.prims(rec) % 3 == 0) & (colors_ref.prims(rec) >= 0) & (colors_ref.prims(rec) < 40) & (colors_ref.prims(rec) != 9)
        assert unchanged.sum() >= 5 and same(got_p[unchanged], pts[unchanged]) and not same(got_p[8], pts[8]) and (got_p[8] == pts[8]).all()
    # each attribute alone: the others' outputs are not produced
    only_n = orc.dress_hits({"nrm_rows": d["nrm_rows"]}, tris, rec, pts)
    assert same(only_n[0], want_n) and only_n[1] is None and only_n[2] is None
    only_c = orc.dress_hits({"col_rows": d["col_rows"]}, tris, rec, pts)
    assert only_c[0] is None and same(only_c[1], colors_ref.hit_colors(order, f, col, rec)) and only_c[2] is None
    only_p = orc.dress_hits({"prev_tris": prev}, tris, rec, pts)
    assert only_p[0] is None and only_p[1] is None and same(only_p[2], got_p)
    no_tex = orc.dress_hits({"uv_rows": d["uv_rows"]}, tris, rec, pts)          # UVs without texels: no texture, so no albedo
    assert no_tex == (None, None, None)


@pytest.mark.parametrize("flags", range(8))
@pytest.mark.parametrize("size", [(1, 1), (3, 5), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_textured_albedo_equals_the_numpy_definitions(orc, size, flags):
    tris, order, f, _, col, uv, _ = _corner_case()
    assert np.nanmin(uv[np.isfinite(uv)]) < -1.4 and np.nanmax(uv[np.isfinite(uv)]) > 2.4                                   # drawn from [-1.5, 2.5]
    rec = _records(257, seed=9)
    tex = mf.random_texture(*size, seed=7)
    host = mf.HostMesh(f)
    host.tris, host.order = tris, order
    for colors in (None, col):                                                  # base 0.85, and the colours' blend
        d = mf.dress(host, 120, colors=colors, uvs=uv, texels=tex, flags=flags)
        _, got, _ = orc.dress_hits(d, tris, rec)
        want = _want_albedo(order, f, colors, uv, tex, flags, rec)
        assert same(got, want), (colors is not None, np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1)))
    assert (got[24:] != 0).any()


# ---------------------------------------------------------------- 3: anchors at the oracle's own level
@functools.lru_cache(maxsize=None)
def _flat_frames():
    """The undressed frames 0 and 1 of the flat scene, GI and AO on, spp 2, cameraMoved = 1."""
    import oracle as orc
    host, _, n = flat_scene()
    faces = scenes.tiny_env(8)
    first, _ = orc.render(mf.uniforms(2, 0, n), host.nodes, host.tris, faces)
    second, _ = orc.render(mf.uniforms(2, 1, n), host.nodes, host.tris, faces, first[0])
    return first, second


def _flat_dresses():
    host, nv, _ = flat_scene()
    white = np.full((5, 3, 4), 255, np.uint8)
    alone = {"normals": mf.dress(host, nv, normals=True),
             "grey": mf.dress(host, nv, colors=np.full((nv, 3), GREY, f32)),
             "white": mf.dress(host, nv, uvs=mf.random_uvs(nv, 4), texels=white, flags=uvs_ref.SRGB),
             "still": {"prev_tris": host.tris.copy()}}
    every = {}
    for d in alone.values():
        every.update(d)
    return dict(alone, together=every)


@pytest.mark.parametrize("which", ["normals", "grey", "white", "still", "together"])
def test_identity_dresses_render_the_undressed_frame(orc, which):
    host, nv, n = flat_scene()
    faces = scenes.tiny_env(8)
    first, second = _flat_frames()
    rec, _ = orc.primary_hits(mf.uniforms(2, 1, n), host.nodes, host.tris)
    hit = colors_ref.prims(rec) >= 0
    assert hit.sum() >= 200 and (~hit).sum() >= 200
    below = host.tris[colors_ref.prims(rec)[hit], 1] == 1
    assert below.sum() >= 100 and (~below).sum() >= 100                         # the floor and the ceiling are both in view
    # the premise of the normals' anchor: (+0, +-1, +0) at every vertex
    rows, vn = mf.normal_rows(host.tris, host.order, host.f, nv)
    want = np.zeros((nv, 3), f32)
    want[:nv // 2, 1], want[nv // 2:, 1] = 1, -1
    assert same(vn, want)
    d = _flat_dresses()[which]
    u0, u1 = mf.uniforms(2, 0, n), mf.uniforms(2, 1, n)
    assert u1.cameraMoved == 1
    got0, _ = orc.render(u0, host.nodes, host.tris, faces, dress=d)
    got1, _ = orc.render(u1, host.nodes, host.tris, faces, got0[0], dress=d)
    for name, x, y in zip(TARGETS, got0 + got1, first + second):
        assert same(x, y), name
    assert (orc.half_to_float(second[0])[..., :3] != 0).any() and not same(first[0], second[0])      # lit, and the history counts


# ---------------------------------------------------------------- 4: the dress does something, and where it should
def _rigid_before():
    """The default placement a small rigid step earlier: turned about y by 0.1 rad and shifted."""
    M = np.asarray(rt.default_bvh_transform(), np.float64).reshape(4, 4).T
    c, s = np.cos(0.1), np.sin(0.1)
    R = np.eye(4)
    R[:3, :3] = [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    R[:3, 3] = [0.05, -0.03, 0.02]
    return np.ascontiguousarray((R @ M).T, f32).reshape(-1)


def test_the_dressed_sphere(orc):
    host, nv, n, pos = sphere_scene()
    f = host.f
    faces = scenes.tiny_env(8)
    u = mf.uniforms(2, 0, n)
    prev = np.zeros_like(host.tris)
    prev[:, COORDS] = rt.gather_triangles(pos, f, _rigid_before())[host.order]
    colors, uvs, tex = mf.random_colors(nv, 6), mf.random_uvs(nv, 12), mf.random_texture(3, 5, 13)
    d = mf.dress(host, nv, normals=True, colors=colors, uvs=uvs, texels=tex)
    d["prev_tris"] = prev
    off, _ = orc.render(u, host.nodes, host.tris, faces)
    on, _ = orc.render(u, host.nodes, host.tris, faces, dress=d)
    rec, pts = orc.primary_hits(u, host.nodes, host.tris)
    hit = colors_ref.prims(rec) >= 0
    assert hit.sum() >= 200 and (~hit).sum() >= 200
    hit2 = hit.reshape(H, W)
    assert same(on[2], off[2]) and ((orc.half_to_float(on[2])[..., 3] != 0) == hit2).all()                   # GPOS: the geometry is the undressed one
    assert same(_half(pts)[hit], on[2].reshape(-1, 4)[hit][:, :3])                                           # ... and primary_hits are the frame's hits
    assert ((on[0] != off[0]).any(axis=2) & hit2).sum() >= 100                                               # COLOR0 follows the dress
    _, vn = mf.normal_rows(host.tris, host.order, f, nv)
    want_n = np.zeros((H * W, 4), np.uint16)
    want_n[:, :3] = _half(np.where(hit[:, None], normals_ref.hit_normals(host.tris, host.order, f, vn, rec), f32(0)))
    assert same(on[3].reshape(-1, 4), want_n)                                                                # GNRM: f16(hit_normals), zeros at misses
    assert (on[3].reshape(-1, 4)[hit] != off[3].reshape(-1, 4)[hit]).any(axis=1).sum() >= 100
    _, mo = motion_ref.hit_motion(u, host.tris, prev, rec, pts)
    want_m = np.where(hit[:, None], _half(mo), FOUR)
    assert same(on[1].reshape(-1, 2), want_m)                                                                # MOTION: f16(hit_motion), (4, 4) at misses
    assert (on[1].reshape(-1, 2)[hit] != off[1].reshape(-1, 2)[hit]).any(axis=1).sum() >= 100
    # each attribute moves its own targets only
    for name, moves in (("nrm_rows", (0, 3)), ("col_rows", (0,)), ("prev_tris", (1,))):
        got, _ = orc.render(u, host.nodes, host.tris, faces, dress={name: d[name]})
        for k, t in enumerate(TARGETS):
            assert same(got[k], off[k]) == (k not in moves), (name, t)
    # frame 1 with history: the resolve reprojects with the object's motion (cameraMoved = 1), so COLOR0 differs from a frame dressed without it
    u1 = mf.uniforms(2, 1, n)
    with_motion, _ = orc.render(u1, host.nodes, host.tris, faces, on[0], dress=d)
    without = dict(d)
    del without["prev_tris"]
    camera_only, _ = orc.render(u1, host.nodes, host.tris, faces, on[0], dress=without)
    assert not same(with_motion[0], camera_only[0]) and same(with_motion[3], camera_only[3])


# ---------------------------------------------------------------- 5: the hybrid scene ignores the dress
def test_hybrid_ignores_the_dress(orc):
    host, nv, n, pos = sphere_scene()
    faces = scenes.tiny_env(8)
    d = mf.dress(host, nv, normals=True, colors=mf.random_colors(nv, 6), uvs=mf.random_uvs(nv, 12), texels=mf.random_texture(3, 5, 13), motion=True)
    assert not same(d["prev_tris"], host.tris)
    for use_bvh in (rt.RT_SCENE_HYBRID, False):
        u = mf.uniforms(2, 0, n, use_bvh=use_bvh)
        off, c0 = orc.render(u, host.nodes, host.tris, faces)
        on, c1 = orc.render(u, host.nodes, host.tris, faces, dress=d)
        for name, x, y in zip(TARGETS, on, off):
            assert same(x, y), (use_bvh, name)
        assert c0.as_tuple() == c1.as_tuple()
    assert c0.hitPixels >= 200


# ---------------------------------------------------------------- 6: independence
def test_the_oracle_never_touches_the_product():
    """The converse of test_c_abi.py::test_product_never_touches_the_oracle: nothing under oracle/ includes, or is built from, the product's sources."""
    seen = 0
    for p in sorted((ROOT / "oracle").iterdir()):
        if p.suffix not in (".cpp", ".c", ".h", ".hpp") and p.name != "Makefile":
            continue
        text = p.read_text()
        seen += 1
        if p.name == "Makefile":
            assert "csrc" not in text and "opengl-raytracing_amd" not in text, p.name
        for line in text.splitlines():
            if re.match(r"\s*#\s*include", line):
                assert "csrc" not in line and "opengl-raytracing_amd" not in line and "rt_mi355" not in line and "rt_mesh" not in line, (p.name, line)
    assert seen >= 6 and (ROOT / "oracle" / "orc_dress.h").exists()
