"""The dynamic-mesh C API after its move to csrc/rt_api_mesh.hip.  Contract: every call of tests/mesh_api_cases.py, in every state it
belongs to, returns the code and leaves the rt_last_error text that tests/golden/mesh_api_parent.json recorded on the commit before the move -- when
four copies of the hit query, their _host twins and the accessors were written out one by one; the UV and texture cases on the commit before colours
and UVs became one corner-attribute path -- and touches no output; the six hit queries give the
same bits through their host and their device entry point, for query sizes that grow and then reuse the one staging buffer, and those bits are the host
definitions'; rt_mesh_hit_parts keeps taking records that are 4-byte aligned only.  Every comparison is exact."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import mesh_api_cases as cases
import opengl_raytracing_amd as rt

pytestmark = pytest.mark.gpu

f32 = np.float32
GOLDEN = json.loads((Path(__file__).resolve().parent / "golden" / "mesh_api_parent.json").read_text())


def _dev():
    return torch.device("cuda", 0)


def _same(x, y):
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))


# ---------------------------------------------------------------- 1: refusals pinned to the parent commit
def test_the_table_is_the_recorded_one():
    assert set(GOLDEN) == set(cases.STATES)
    for state in cases.STATES:
        assert set(GOLDEN[state]) == {name for name, (_, states) in cases.CALLS.items() if state in states}, state


@pytest.mark.parametrize("state", cases.STATES)
def test_refusals_are_the_parents(state):
    got, want = cases.run(state), GOLDEN[state]
    assert set(got) == set(want)
    for name, g in got.items():
        w = dict(want[name])
        assert (g["rc"], g["error"]) == (w["rc"], w["error"]), (state, name, g, w)
        assert g.get("untouched", True), (state, name, "an output was written")
        if name == "rt_mesh_positions" and g["rc"] != rt.RT_OK:      # the one accessor that did not clear its outputs on refusal: either is accepted
            g, w = dict(g), w
            g.pop("cleared"), w.pop("cleared")
        assert g == w, (state, name, g, w)


# ---------------------------------------------------------------- 2: the four queries through both entry points, sharing one staging buffer
def _posed(b):
    """The table's mesh with everything on, skinned one step and refitted, its colours and UVs set; -> what the host definitions need."""
    v, f = cases.mesh()
    cases.enter(b, "all_on")
    b.mesh_set_colors(np.random.default_rng(7).uniform(0.05, 1.0, v.shape).astype(f32))
    b.mesh_set_uvs(np.random.default_rng(8).uniform(-1.0, 2.0, (v.shape[0], 2)).astype(f32))   # past [0, 1): the texture repeats
    a = 0.4
    turned = np.eye(4)
    turned[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    b.mesh_set_bones(np.stack([np.eye(4, dtype=f32).reshape(-1), np.ascontiguousarray(turned.T, f32).reshape(-1)]))
    b.mesh_skin()
    b.mesh_refit_parts()
    b.synchronize()
    n = cases.N_TRIS
    tris = b.debug_read_scene("tris").view(f32).reshape(-1, 12)[:n].copy()
    prev = b.mesh_prev_tris()
    assert not _same(tris, prev)                                    # the skin step moved the mesh
    normals, colors, uvs = (a().cpu().numpy().copy() for a in (b.mesh_vertex_normals, b.mesh_colors, b.mesh_uvs))
    return f, tris, prev, b.mesh_order(as_torch=False).copy(), normals, colors, uvs


def _parts_of(prim, order):
    """(part, triangle within the part) of each prim, as mesh_parts() and mesh_order() imply; (-1, -1) for a miss."""
    first = np.asarray(cases.PART_FIRST)
    hit = prim >= 0
    tri = order[np.where(hit, prim, 0)]
    part = np.searchsorted(first, tri, side="right") - 1
    return np.where(hit, part, -1).astype(np.int32), np.where(hit, tri - first[part], -1).astype(np.int32)


def test_queries_agree_across_their_two_paths():
    rng = np.random.default_rng(11)
    with rt.Renderer() as b:
        f, tris, prev, order, normals, colors, uvs = _posed(b)
        assert np.array_equal(b.mesh_parts(), cases.PART_FIRST)
        k = np.arange(64) % cases.N_TRIS                            # rays aimed at triangle centroids from around the mesh, every seventh reversed
        target = (tris[k, 0:3] + (tris[k, 4:7] + tris[k, 8:11]) / 3).astype(f32)
        org = (target + rng.normal(0, 1, target.shape) * 4).astype(f32)
        dirs = target - org
        dirs = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(f32)
        dirs[::7] = -dirs[::7]
        rows = np.arange(5000) % 64                                 # 5000 rays: the 64 repeated
        org, dirs = np.ascontiguousarray(org[rows]), np.ascontiguousarray(dirs[rows])
        for m in (1, 64, 65, 5000, 3):                              # the staging buffer grows, then is reused oversize
            r = b.trace_rays(org[:m], dirs[:m])
            rec, hit = r.record, r.prim >= 0
            if m == 5000:
                assert hit[:64].any() and not hit[:64].all()
            pts = (org[:m] + dirs[:m] * np.where(hit, r.t, 0).astype(f32)[:, None]).astype(f32)
            d_rec, d_pts = torch.from_numpy(rec).to(_dev()), torch.from_numpy(pts).to(_dev())
            host = {"parts": b.mesh_hit_parts(rec), "prev": b.mesh_hit_prev_points(rec, pts), "normals": b.mesh_hit_normals(rec), "colors": b.mesh_hit_colors(rec),
                    "uvs": b.mesh_hit_uvs(rec), "texels": b.mesh_hit_texels(rec)}
            dev = {"parts": b.mesh_hit_parts(d_rec), "prev": b.mesh_hit_prev_points(d_rec, d_pts), "normals": b.mesh_hit_normals(d_rec), "colors": b.mesh_hit_colors(d_rec),
                   "uvs": b.mesh_hit_uvs(d_rec), "texels": b.mesh_hit_texels(d_rec)}
            torch.cuda.synchronize()
            for q in ("prev", "normals", "colors", "uvs", "texels"):
                assert _same(host[q], dev[q].cpu().numpy()), (m, q)
            for i in (0, 1):
                assert _same(host["parts"][i], dev["parts"][i].cpu().numpy()), (m, "parts", i)
            assert _same(host["prev"], rt.hit_motion(None, tris, prev, rec, pts, want=("prev",))[0]), m
            assert _same(host["normals"], rt.hit_normals(tris, order, f, normals, rec)), m
            assert _same(host["colors"], rt.hit_colors(tris, order, f, colors, rec)), m
            assert _same(host["uvs"], rt.hit_uvs(order, f, uvs, rec)), m
            assert _same(host["texels"], np.where(hit[:, None], rt.sample_texture(cases.texture(), 0, host["uvs"]), f32(0)).astype(f32)), m   # a miss: zeros
            want = _parts_of(r.prim, order)
            assert _same(host["parts"][0], want[0]) and _same(host["parts"][1], want[1]), m


def test_hit_parts_takes_records_aligned_to_four_bytes():
    """Seven records that start 4 bytes into a buffer of eight: the device entry reads words, not whole records, and keeps accepting them."""
    with rt.Renderer() as b:
        order = _posed(b)[3]
        words = np.zeros(32, np.int32)                              # 8 records; read from word 1: record j = words[1 + 4j : 5 + 4j], prim its second word
        prims = np.array([0, 64, 7, -1, 33, 65, 29], np.int32)      # rows of both parts, a miss, a prim outside the mesh
        words[2:30:4] = prims
        buf = torch.from_numpy(words).to(_dev())
        parts, tris = (torch.full((7,), -7, dtype=torch.int32, device=_dev()) for _ in range(2))
        torch.cuda.synchronize()
        rc = rt.lib().rt_mesh_hit_parts(b._h, C.c_void_p(buf.data_ptr() + 4), 7, C.c_void_p(parts.data_ptr()), C.c_void_p(tris.data_ptr()))
        assert rc == rt.RT_OK, rt.lib().rt_last_error(b._h)
        b.synchronize()
        rec = np.ascontiguousarray(words[1:29]).view(f32).reshape(7, 4)
        want = b.mesh_hit_parts(rec)
        assert _same(parts.cpu().numpy(), want[0]) and _same(tris.cpu().numpy(), want[1])
        inside = _parts_of(np.where(prims < cases.N_TRIS, prims, -1), order)
        assert _same(want[0], inside[0]) and _same(want[1], inside[1])
