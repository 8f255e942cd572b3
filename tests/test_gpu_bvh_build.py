"""rt_build_bvh_gpu (csrc/rt_bvh_gpu.hip): the reference's median-split builder on the device.  Against the host builder
(= the oracle's, tests/test_host_parity.py) on tie-free input: identical node numbering, links, leaf ranges and boxes, and the
same SET of triangles in every leaf.  Against its own definition (tests/bvh_build_ref.py; the whole corpus: tests/test_gpu_bvh_corpus.py)
on the meshes whose medians tie: every word of nodes12 and tris12.  A frame rendered from the GPU-built arrays equals the oracle's
frame from the same arrays bit for bit."""
import time

import numpy as np
import pytest

import bvh_build_ref as ref
import opengl_raytracing_amd as rt
import scenes

pytestmark = pytest.mark.gpu


def _compare(nodes_g, tris_g, nodes_c, tris_c):
    assert nodes_g.shape == nodes_c.shape and tris_g.shape == tris_c.shape
    assert np.array_equal(nodes_g[:, [3, 7, 8, 9]], nodes_c[:, [3, 7, 8, 9]])              # links, first, count
    assert np.array_equal(nodes_g[:, [0, 1, 2, 4, 5, 6]], nodes_c[:, [0, 1, 2, 4, 5, 6]])  # boxes, bit for bit
    leaves = np.where(nodes_c[:, 9] > 0)[0]
    for i in leaves:
        f, c = int(nodes_c[i, 8]), int(nodes_c[i, 9])
        a = sorted(map(tuple, tris_g[f:f + c]))
        b = sorted(map(tuple, tris_c[f:f + c]))
        assert a == b, i


def _check_valid(nodes, tris, t9):
    """A well-formed tree of the reference's shape over exactly the input triangles, whatever the tie-breaking."""
    left, right = nodes[:, 3].astype(int), nodes[:, 7].astype(int)
    first, cnt = nodes[:, 8].astype(int), nodes[:, 9].astype(int)
    inner = cnt == 0
    assert np.array_equal(np.minimum(nodes[left[inner], 0:3], nodes[right[inner], 0:3]), nodes[inner, 0:3])     # parent = union of children
    assert np.array_equal(np.maximum(nodes[left[inner], 4:7], nodes[right[inner], 4:7]), nodes[inner, 4:7])
    v0, v1, v2 = tris[:, 0:3], tris[:, 0:3] + tris[:, 4:7], tris[:, 0:3] + tris[:, 8:11]
    tmin, tmax = np.minimum(v0, np.minimum(v1, v2)), np.maximum(v0, np.maximum(v1, v2))
    for i in np.where(~inner)[0]:
        sl = slice(first[i], first[i] + cnt[i])
        assert np.array_equal(tmin[sl].min(0), nodes[i, 0:3]) and np.array_equal(tmax[sl].max(0), nodes[i, 4:7]), i
    assert sorted(map(tuple, tris[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]])) == sorted(map(tuple, t9))                   # a permutation of the input


def _equals_the_definition(nodes, tris, t9):
    """Every word of both arrays against tests/bvh_build_ref.py: numbering, links, boxes with the sign of their zeros, the rows inside the leaves."""
    nr, tr, _ = ref.ref_build(t9)
    assert nodes.shape == nr.shape and tris.shape == tr.shape
    for name, got, want in (("nodes12", nodes, nr), ("tris12", tris, tr)):
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert bad.size == 0, f"{name}: {bad.shape[0]} words differ, first at row {bad[0][0]} column {bad[0][1]}"


@pytest.mark.parametrize("n", [1, 8, 9, 17, 100, 1000, 20480])
def test_gpu_builder_equals_the_host_builder(n):
    rng = np.random.default_rng(n)
    t9 = rng.normal(0, 1, (n, 9)).astype(np.float32)
    t9[:, 3:] *= 0.1
    with rt.Renderer() as r:
        ng, tg = r.build_bvh_gpu(t9)
    nc, tc = rt.build_bvh(t9)
    _compare(ng, tg, nc, tc)
    _equals_the_definition(ng, tg, t9)


def test_gpu_builder_on_the_bench_mesh_and_render_parity(orc):
    v, f = rt.meshgen.bunny_standin(5)
    t9 = rt.gather_triangles(v, f)
    with rt.Renderer() as r:
        t0 = time.perf_counter()
        ng, tg = r.build_bvh_gpu(t9)
        t_gpu = time.perf_counter() - t0
        t0 = time.perf_counter()
        nc, tc = rt.build_bvh(t9)
        t_cpu = time.perf_counter() - t0
        # the icosphere-based mesh has equal centroid keys (symmetry), so medians tie and the host's nth_element may split such
        # ranges differently: same skeleton, a valid tree -- and exactly the tree of the definition, whose stable sort decides the ties
        assert np.array_equal(ng[:, [3, 7, 8, 9]], nc[:, [3, 7, 8, 9]])
        _check_valid(ng, tg, t9)
        same_box = np.all(ng[:, [0, 1, 2, 4, 5, 6]] == nc[:, [0, 1, 2, 4, 5, 6]], axis=1)
        print(f"build {t9.shape[0]} triangles: GPU {t_gpu * 1e3:.1f} ms, host {t_cpu * 1e3:.1f} ms; boxes identical to the host build: {same_box.mean() * 100:.1f} %")
        _equals_the_definition(ng, tg, t9)
        W, H = 120, 80
        faces = scenes.tiny_env(8)
        p = rt.default_render_params()
        p.sppPerFrame = 2
        cam = scenes.camera("closeup", aspect=W / H)
        r.upload_bvh(ng, tg)
        r.upload_env(faces)
        r.resize(W, H)
        prev = None
        for frame in range(2):
            u = rt.frame_uniforms(p, cam, W, H, frame, True, ng.shape[0], tg.shape[0])
            r.render_frame(u)
            want, _ = orc.render(u, ng, tg, faces, prev)
            for g, w_, name in zip(r.read_all(), want, ("color", "motion", "gpos", "gnrm")):
                assert np.array_equal(g, w_), (frame, name)
            prev = want[0]


def test_gpu_builder_million_triangles():
    v, f = rt.meshgen.million_triangle_scene()
    t9 = rt.gather_triangles(v, f, np.eye(4, dtype=np.float32).reshape(-1))
    with rt.Renderer() as r:
        r.build_bvh_gpu(t9[:1000])          # warm-up: code object load
        t0 = time.perf_counter()
        ng, tg = r.build_bvh_gpu(t9)
        t_gpu = time.perf_counter() - t0
    t0 = time.perf_counter()
    nc, tc = rt.build_bvh(t9)
    t_cpu = time.perf_counter() - t0
    print(f"build {t9.shape[0]} triangles: GPU {t_gpu * 1e3:.1f} ms (incl. host<->device copies), host {t_cpu * 1e3:.1f} ms")
    assert np.array_equal(ng[:, [3, 7, 8, 9]], nc[:, [3, 7, 8, 9]])
    same_box = np.all(ng[:, [0, 1, 2, 4, 5, 6]] == nc[:, [0, 1, 2, 4, 5, 6]], axis=1)
    print(f"boxes identical to the host build: {same_box.mean() * 100:.2f} %")      # information: they differ below a median where centroids tie
    _equals_the_definition(ng, tg, t9)                  # every box, leaf boxes included, and every row
    inner = ng[:, 9] == 0
    left, right = ng[:, 3].astype(int), ng[:, 7].astype(int)
    assert np.array_equal(np.minimum(ng[left[inner], 0:3], ng[right[inner], 0:3]), ng[inner, 0:3])
    assert np.array_equal(np.maximum(ng[left[inner], 4:7], ng[right[inner], 4:7]), ng[inner, 4:7])
    a = np.ascontiguousarray(tg[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]).view([("", np.float32)] * 9).ravel()
    b = np.ascontiguousarray(t9).view([("", np.float32)] * 9).ravel()
    assert np.array_equal(np.sort(a), np.sort(b))       # a permutation of the input
