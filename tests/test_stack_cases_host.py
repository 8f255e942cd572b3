"""The conditions that keep tests/test_gpu_walk_stacks.py honest, on the CPU: the fixtures of stack_cases.py really send every ray through
every box, the plain-Python models of the walks really reach the bound of each stack on them, the answers known by construction are the oracle's, and
-- for every scene and every option set the suite uploads -- the stack rt.trace_build hands an any-hit launch is at least the need of the tree that
build walks.

What the models say (the table of DESIGN.md 27 is printed by test_model_peaks with -s):
  closest-hit   peak = depth - 1 on a ladder walked from beyond its far end (the leaf is the far child at every level) and on the slabs; the launch has
                `depth` entries (at least 4): one spare.
  any-hit       the plain four-wide walk -- the walk any_stack_need bounds -- peaks at anyStack exactly on every fixture.  k_trace and k_trace_packets
                keep the first leaf they meet in a register and not on the stack, so their own peak is anyStack - 1 or anyStack: a register holds one
                leaf, the plain walk would have stacked it.
"""
import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scene_pack_cases
import scenes
import stack_cases as sc
import test_gpu_options as gpu_options
import trace_build_cases

FIXTURES = [fx.name for fx in sc.fixtures()]
f32 = np.float32


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in gpu_options.OPTION_VARS:
        monkeypatch.delenv(v, raising=False)


def _packed(fx, **options):
    return rt.pack_scene(fx.nodes, fx.tris, **(options or {"qnodes": -1}))


# ---------------------------------------------------------------- 1: every ray enters every box, with a margin

@pytest.mark.parametrize("name", FIXTURES)
def test_every_ray_enters_every_box_with_a_margin(name):
    """In float64, on the float32 rays as the device gets them: every ray (single and packet) enters every binary node box and every child box of the
    four-wide records, stays at least 1/256 of the box's extent inside its y-z cross-section over the box's x range, and passes every rung at least
    EDGE_MARGIN from the rung's nearest edge, on the side of the hypotenuse the construction says."""
    fx = sc.by_name(name)
    lo4, hi4, ref4 = sc.wide4(_packed(fx))
    present = ref4.reshape(-1) != sc.NO_CHILD
    boxes = [(fx.nodes[:, 0:3], fx.nodes[:, 4:7]), (lo4.reshape(-1, 3)[present], hi4.reshape(-1, 3)[present])]
    assert not np.isnan(boxes[1][0]).any() and np.isnan(lo4.reshape(-1, 3)[~present]).all()
    for r in (sc.rays(fx), sc.packet_rays(fx)):
        o, d = r.org.astype(np.float64), r.dirs.astype(np.float64)
        for lo, hi in boxes:
            t_in, t_out = sc.slab64(o, d, lo.astype(np.float64), hi.astype(np.float64))
            assert (t_out >= t_in).all() and (t_in > 0).all()                     # entered, from outside
            assert sc.box_margin(r, lo, hi).min() >= 1.0 / 256.0
        margin, inside = sc.edge_margin(fx, r)
        assert margin.min() >= sc.EDGE_MARGIN[fx.kind], margin.min()
        k = np.arange(fx.n + 1)[None]
        assert np.array_equal(inside, (k >= r.lo[:, None]) & (k <= r.hi[:, None]))
        assert (r.hits == 0).any() and (r.hits == fx.n + 1).any()                 # j = -1 and j = n are there
        assert (r.tmax > 0).all()
    r = sc.rays(fx)
    if fx.n + 2 <= 64:                   # every run of 64 rays of a family holds every rung
        for s in range(0, r.j.size, 64):
            assert set(r.j[s:s + 64]) == set(range(-1, fx.n + 1)), s
    pk = sc.packet_rays(fx)
    assert (pk.org.reshape(-1, 4, 3) == pk.org.reshape(-1, 4, 3)[:, :1]).all()
    assert (np.diff(np.sort(pk.lo.reshape(-1, 4) + pk.hi.reshape(-1, 4), axis=1), axis=1) != 0).all()     # four different crossings


# ---------------------------------------------------------------- 2: the models reach the bounds

def _peaks(fx):
    """-> dict of the modelled peaks over the rays that hit nothing within their limit (a hit ends an any-hit walk early) and, closest-hit, over the
    rays of rungs -1, 0 and n."""
    p = _packed(fx)
    w4 = sc.wide4(p)
    r = sc.rays(fx)
    free = np.flatnonzero(~r.occluded)
    out = {"anyStack": int(p["info"].anyStack), "depth": int(p["info"].treeDepth), "any": 0, "any_register": 0, "any_near": 0, "closest": {}}
    for i in free:
        out["any"] = max(out["any"], sc.any_model(w4, r.org[i], r.dirs[i], r.tmax[i])[0])
        out["any_register"] = max(out["any_register"], sc.any_model(w4, r.org[i], r.dirs[i], r.tmax[i], register=True)[0])
        out["any_near"] = max(out["any_near"], sc.any_model(w4, r.org[i], r.dirs[i], r.tmax[i], register=True, near=True)[0])
        assert sc.any_model(w4, r.org[i], r.dirs[i], r.tmax[i])[1] == fx.nodes[fx.nodes[:, 9] > 0].shape[0]           # it met every leaf
    for fam in range(4):
        sel = np.flatnonzero((r.family == fam) & np.isin(r.j, (-1, 0, fx.n)))
        out["closest"][fam] = max(sc.closest_model(fx, r.org[i], r.dirs[i])[2] for i in sel)
    return out


@pytest.mark.parametrize("name", FIXTURES)
def test_model_peaks(name):
    fx = sc.by_name(name)
    pk = _peaks(fx)
    assert pk["depth"] == fx.depth
    assert pk["anyStack"] == sc.any_stack_need(sc.wide4(_packed(fx))[2])            # the Python restatement of any_stack_need
    if fx.kind == "slab":
        assert pk["anyStack"] == {3: 4, 6: 9, 7: 10}[fx.depth - 1]
    # any-hit: the plain walk reaches the bound exactly; the kernels' walk keeps one leaf in a register
    assert pk["any"] == pk["anyStack"]
    assert pk["anyStack"] - 1 <= pk["any_register"] <= pk["anyStack"]
    assert pk["anyStack"] - 1 <= pk["any_near"] <= pk["anyStack"]
    # closest-hit: one entry per level below the root where the leaf is the far child (ladders: the rays that travel towards -x) and on the slabs
    far_leaf = (0, 2) if fx.kind == "ladder" else (0, 1, 2, 3)
    for fam in far_leaf:
        assert pk["closest"][fam] == fx.depth - 1, (fam, pk["closest"])
    # the launches: what rt.trace_build hands out holds the peaks
    forms = tuple(f for f, a in trace_build_cases.FORM_ARRAYS.items() if _packed(fx)[a].size)
    b_any = rt.trace_build(True, depth=fx.depth, any_stack=pk["anyStack"], forms=forms)
    b_closest = rt.trace_build(False, depth=fx.depth, any_stack=pk["anyStack"], forms=forms)
    assert b_any.stack == max(4, pk["anyStack"]) >= pk["any"] and b_closest.stack == max(4, fx.depth) > max(pk["closest"].values())
    mega = 16 if fx.depth <= 16 else 24 if fx.depth <= 24 else 32                   # csrc/rt_mega.hip launch_depth
    assert mega > fx.depth - 1 and min(max(fx.depth, 1), 64) > fx.depth - 1         # ... and rt_query_stack_entries
    print(f"| {fx.name} | {fx.depth} | {pk['anyStack']} | {b_closest.stack} / {b_any.stack} / {mega} | {max(pk['closest'].values())} / {pk['any']} / {pk['any_register']} |")


@pytest.mark.parametrize("D", sc.SLAB_DEPTHS)
def test_implicit_topology_peaks(D):
    """The implicit four-wide topology of a slab (what RT_IMPLICIT's any-hit build walks): its need by the formula, by any_stack_need over the topology,
    and the plain walk's peak on it are one number, and pack_scene's anyStack -- of the collapsed tree -- equals it."""
    fx = sc.slab(D)
    p = _packed(fx, implicit=True)
    assert p["info"].implicitDepth == D and p["impl_nodes4"].size
    i4 = sc.implicit4(fx)
    need = sc.implicit_need(D)
    assert sc.any_stack_need(i4[2]) == need == p["info"].anyStack
    r = sc.rays(fx)
    free = np.flatnonzero(~r.occluded)
    assert max(sc.any_model(i4, r.org[i], r.dirs[i], r.tmax[i])[0] for i in free) == need


# ---------------------------------------------------------------- 3: the constructed answers are the oracle's

@pytest.mark.parametrize("name", FIXTURES)
def test_constructed_answers_equal_the_oracle(orc, name):
    fx = sc.by_name(name)
    r = sc.rays(fx)
    prim, t, occ = sc.oracle_answers(fx)
    hit = r.first >= 0
    assert np.array_equal(prim[hit], fx.row[r.first[hit]]) and (prim[~hit] == -1).all()
    # t: tvec.x / -rd.x in float32 -- a subtraction, a reciprocal and a product, half an ulp each: within 2 ulp of the float64 value, 4 allowed
    assert (np.abs(t[hit].astype(np.float64) - r.t_first[hit]) <= 4 * np.finfo(f32).eps * r.t_first[hit]).all()
    assert np.array_equal(occ, r.occluded)
    assert np.array_equal(sc.oracle_packet_answers(fx), sc.packet_rays(fx).occluded)
    # the model of the closest-hit walk gives the oracle's bits on a sample of the rays
    for i in range(0, r.org.shape[0], 16):
        tri, tm, _ = sc.closest_model(fx, r.org[i], r.dirs[i])
        assert tri == prim[i] and (tri < 0 or tm.view(np.uint32) == t[i].view(np.uint32)), i
    # the rays that hit everything, through the multi-hit definition: every rung, nearest first
    full = np.flatnonzero(r.hits == fx.n + 1)
    mh = rt.multi_hits(fx.nodes, fx.tris, r.org[full], r.dirs[full], max_hits=32)
    assert (mh.count == fx.n + 1).all()
    k = min(32, fx.n + 1)
    forward = r.dirs[full, 0] > 0
    want = np.where(forward[:, None], np.arange(k)[None], fx.n - np.arange(k)[None])
    assert np.array_equal(mh.prim[:, :k], fx.row[want]) and (mh.prim[:, k:] == -1).all()


# ---------------------------------------------------------------- 4: the stack of an any-hit launch holds the tree the launch walks

def _parity_meshes():
    """The meshes of tests/test_gpu_parity.py, by its own recipes."""
    rng = np.random.default_rng(3)
    out = {"one_leaf": scenes.one_leaf_mesh(), "tiny": scenes.bunny_bvh(0), "bunny3": scenes.bunny_bvh(3), "deep": scenes.bunny_bvh(4)}
    for name, n in (("ragged", 1100), ("odd_counts", 1400), ("odd_depth", 700)):
        c = (np.array([-2.0, 1.5, 0.0]) + rng.uniform(-0.5, 0.5, (n, 3))).astype(f32)
        t9 = np.concatenate([c, c + rng.uniform(-0.08, 0.08, (n, 3)).astype(f32), c + rng.uniform(-0.08, 0.08, (n, 3)).astype(f32)], axis=1).astype(f32)
        out[name] = rt.build_bvh(t9)
    return out


def _option_sets():
    """name -> (environment, stats): every environment of trace_build_cases (the ray, frame and instrumented cases of test_gpu_options.py), those of the
    scene-pack checks, and RT_IMPLICIT=1 with RT_ANYHIT_TREE=sah."""
    out = {"none": ({}, False), "implicit_sah": ({"RT_IMPLICIT": "1", "RT_ANYHIT_TREE": "sah"}, False),
           "implicit_sah_qnodes2": ({"RT_IMPLICIT": "1", "RT_ANYHIT_TREE": "sah", "RT_QNODES": "2"}, False)}
    for cid, (_, env, _, _) in gpu_options.RAY_CASES.items():
        out[f"ray/{cid}"] = (env, False)
    for cid, (env, *_) in gpu_options.FRAME_CASES.items():
        out[f"frame/{cid}"] = (env, False)
    for cid, (env, *_) in gpu_options.PACKET_AO_CASES.items():
        out[f"packet_ao/{cid}"] = (dict(env, RT_PACKET_AO="1"), False)
    for cid, (env, _, _) in trace_build_cases.INSTRUMENTED.items():
        out[f"instrumented/{cid}"] = (env, True)
    for cid, (env, _) in {**scene_pack_cases.OPTION_SETS, **scene_pack_cases.OPTIONAL_SETS}.items():
        out[f"pack/{cid}"] = (env, False)
    return out


def _need_of_the_tree_walked(packed, build):
    """any_stack_need of the topology the any-hit build `build` walks on the packed scene."""
    info = packed["info"]
    if build.nodes in ("iN4", "iQ4"):
        assert info.implicitDepth > 0
        return sc.implicit_need(info.implicitDepth)
    assert build.nodes in ("w4", "q4")
    if info.rootRef4 != 0:               # a single leaf: nothing is walked
        return 0
    ref = sc.wide4(packed)[2]
    if build.nodes == "q4":              # the quantised records carry the same references (their fourth 16-byte piece)
        assert np.array_equal(packed["qnodes4"].view(np.int32).reshape(-1, 16)[:, 12:16], ref)
    return sc.any_stack_need(ref)


def test_no_four_wide_tree_over_the_leaves_needs_less_than_the_implicit_one():
    """Why the property below holds under RT_IMPLICIT=1 with RT_ANYHIT_TREE=sah, whatever the mesh: both four-wide builders give a node fewer than four
    children only where all of them are leaves, so a tree whose need is S has at most f(S) leaves, f(0) = 1, f(1) = 2, f(2) = 3, f(S) = 4 f(S - 3) -- and
    f(implicit_need(D) - 1) < 2^D: no tree over the 2^D leaves of a perfect tree needs fewer entries than its implicit topology."""
    f = [1, 2, 3]
    while len(f) < 40:
        f.append(max(4 * f[-3], f[-1]))
    for D in range(1, 24):               # (pack_implicit takes leaf depths up to 23)
        assert f[sc.implicit_need(D) - 1] < 2 ** D <= f[sc.implicit_need(D)], D


def test_the_frames_camera_looks_down_the_whole_ladder(orc):
    """The camera of test_gpu_walk_stacks' frames: the first rung a pixel sees ranges over more than half the ladder, the deep end included."""
    import test_gpu_walk_stacks as gpu
    for name in ("ladder5R", "ladder32L"):
        fx = sc.by_name(name)
        us, _, hit_pixels = gpu._oracle_frames(name, True)
        rec, _ = orc.primary_hits(us[0], fx.nodes, fx.tris)
        prim = rec.view(np.int32)[:, 1]
        seen = set(fx.rung[prim[prim >= 0]].tolist())
        assert len(seen) > (fx.n + 1) // 2 and min(seen) <= fx.n // 8 + 1 and min(hit_pixels) > gpu.W * gpu.H // 2, (name, sorted(seen), hit_pixels)


def test_any_hit_stack_holds_the_tree_the_build_walks():
    """For every scene and option set: the stack rt.trace_build returns for an any-hit launch (k_trace_packets launches with the same) is at least
    any_stack_need of the tree that build walks -- for IMPL builds the implicit four-wide topology, three pushes per full even level and one where
    d + 1 == D, whatever tree anyStack was computed for (under RT_ANYHIT_TREE=sah: the SAH tree)."""
    meshes = {**{fx.name: (fx.nodes, fx.tris) for fx in sc.fixtures()}, **_parity_meshes()}
    # the variables a packer or the build choice reads; the scheduler's make no difference here, so option sets that agree on these are one
    reads = set(scene_pack_cases.PACK_VARS) | {"RT_COOP", "RT_NEAR_FIRST", "RT_LEAFB", "RT_LEAFB_CLOSEST", "RT_TRACE_TIMING", "RT_TRACE_STATS"}
    distinct = {}
    for oname, (env, stats) in _option_sets().items():
        key = (tuple(sorted((k, v) for k, v in env.items() if k in reads)), stats)
        distinct.setdefault(key, oname)
    assert len(distinct) >= 15
    packs = {}
    short, impl_sah = [], 0
    for (env_items, stats), oname in distinct.items():
        env = dict(env_items)
        pack_env = tuple(sorted((k, v) for k, v in env.items() if k in scene_pack_cases.PACK_VARS))
        for mname, (nodes, tris) in meshes.items():
            def one():
                if (mname, pack_env) not in packs:
                    packs[mname, pack_env] = rt.pack_scene(nodes, tris)
                p = packs[mname, pack_env]
                forms = tuple(f for f, a in trace_build_cases.FORM_ARRAYS.items() if p[a].size)
                b = rt.trace_build(True, depth=p["info"].treeDepth, stats=stats, any_stack=p["info"].anyStack, forms=forms)
                return p, b, _need_of_the_tree_walked(p, b)
            p, b, need = trace_build_cases.with_env(env, one)
            impl_sah += "IMPL" in b.bits and not p["info"].collapsed4
            if b.stack < need:
                short.append((oname, mname, b.nodes, b.stack, need))
    assert not short, short
    assert impl_sah >= 3          # the slabs at least take the implicit build over the SAH tree: the combination was looked at
