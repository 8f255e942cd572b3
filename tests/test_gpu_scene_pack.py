"""The device holds what the host packers made (csrc/rt_scene_pack.cpp): after upload_bvh every one of the thirteen scene arrays, the empty
ones included, equals rt.pack_scene's byte for byte and RtSceneInfo agrees with the packer's scalars -- under the default, every RT_QNODES setting,
RT_ANYHIT_TREE=sah, RT_FUSED and RT_IMPLICIT.  An upload that fails leaves the empty scene behind, and the next valid one renders as usual."""
import numpy as np
import pytest

import opengl_raytracing_amd as rt
import scene_pack_cases as cases
import scenes
from test_scene_pack_host import _scene_info

pytestmark = pytest.mark.gpu

MESHES = tuple(f"plain_{n}" for n in (1, 9, 17, 40, 1000))
SETS = {**cases.OPTION_SETS, **cases.OPTIONAL_SETS}
ARRAYS = tuple(rt.SCENE_ARRAYS) + tuple(rt.SCENE_ARRAYS_OPTIONAL)


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in cases.PACK_VARS:
        monkeypatch.delenv(v, raising=False)


@pytest.mark.parametrize("oname", list(SETS))
def test_the_device_holds_what_the_packer_made(monkeypatch, oname):
    env, kw = SETS[oname]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    present = set()
    with rt.Renderer() as r:
        for mname in MESHES:
            nodes, tris = cases.mesh(mname)
            want = rt.pack_scene(nodes, tris, **kw)
            r.upload_bvh(nodes, tris)
            for name in ARRAYS:
                got = r.debug_read_scene(name)
                assert got.size == want[name].size and np.array_equal(got, want[name]), (mname, name, got.size, want[name].size)
                if got.size:
                    present.add(name)
            info = r.scene_info()
            assert {f: int(getattr(info, f)) for f in cases.INFO_FIELDS} == _scene_info(want["info"], want), mname
    # the option did what it is for: a test that passes because every array was empty on both sides is worth nothing
    assert set(rt.SCENE_ARRAYS) - {"qnodes4", "leafbox"} <= present
    assert ({"qnodes4", "leafbox"} <= present) == ("qnodes" in kw and kw["qnodes"] > 0)
    assert ("fused" in present) == bool(kw.get("fused"))
    assert ({"impl_nodes2", "impl_pairs", "impl_nodes4"} <= present) == bool(kw.get("implicit"))
    assert ({"impl_qnodes4", "impl_leafbox"} <= present) == (bool(kw.get("implicit")) and kw.get("qnodes", -1) > 0)


def _empty(r):
    info = r.scene_info()
    return all(int(getattr(info, f)) == 0 for f in cases.INFO_FIELDS) and all(r.debug_read_scene(name).size == 0 for name in ARRAYS)


def test_a_failed_upload_leaves_the_empty_scene(monkeypatch, orc):
    monkeypatch.setenv("RT_QNODES", "2")     # the setting under which the packers have scene fields to write before they get to the depth
    W, H = 96, 64
    nodes, tris = scenes.bunny_bvh(3)
    deep_nodes, deep_tris = cases.chain(33)
    faces = scenes.tiny_env(16)
    cam = scenes.camera("closeup", aspect=W / H)
    with rt.Renderer() as r:
        assert _empty(r)
        r.upload_bvh(nodes, tris)
        assert not _empty(r) and r.debug_read_scene("qnodes4").size > 0
        with pytest.raises(rt.RtError) as e:
            r.upload_bvh(deep_nodes, deep_tris)
        assert e.value.code == rt.RT_ERR_UNSUPPORTED and "tree depth 34" in str(e.value)
        assert _empty(r)
        # a following valid upload renders as usual
        r.upload_bvh(nodes, tris)
        r.upload_env(faces)
        r.resize(W, H)
        u = rt.frame_uniforms(rt.default_render_params(), cam, W, H, 0, True, nodes.shape[0], tris.shape[0])
        r.render_frame(u)
        want, _ = orc.render(u, nodes, tris, faces, None)
        for g, w, name in zip(r.read_all(), want, ("color", "motion", "gpos", "gnrm")):
            st = orc.compare(g, w)
            assert st["bit_diff"] == 0, (name, st)
