"""What every GPU query test sets up: the option variables cleared from the environment before each test, the two pipelines by name, and numpy <->
torch on device 0.  A test module gets the autouse fixture by importing `_clean_env` by name: pytest finds fixtures in the module's namespace."""
import numpy as np
import pytest

import opengl_raytracing_amd as rt

OPTION_VARS = ("RT_COOP", "RT_FUSED", "RT_IMPLICIT", "RT_NEAR_FIRST", "RT_QNODES", "RT_QNODES_SPARSE_BOXES", "RT_ANYHIT_TREE", "RT_LEAFB",
               "RT_LEAFB_CLOSEST", "RT_QUAD_REFILL", "RT_REFILL_MIN", "RT_GUIDED", "RT_CHUNK", "RT_MIN_SEARCH", "RT_REVERSE", "RT_DENSE_TAKE",
               "RT_TRACE_STATS", "RT_TRACE_TIMING", "RT_DEBUG_SKIP_TRAVERSAL", "RT_NEAREST_FAR_FIRST")
PIPELINES = {"megakernel": rt.RT_PIPELINE_MEGAKERNEL, "wavefront": rt.RT_PIPELINE_WAVEFRONT}


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for v in OPTION_VARS:
        monkeypatch.delenv(v, raising=False)


def dev():
    import torch
    return torch.device("cuda", 0)


def to(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, copy=True, order="C")).to(dev())      # (the shared fixtures are read-only)


def np_of(a):
    return a if a is None or isinstance(a, np.ndarray) else a.cpu().numpy()
