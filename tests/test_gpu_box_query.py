"""Box queries on the GPU (rt_query_boxes): every answer against rt.box_overlaps -- the host definition, itself pinned to its numpy
restatement in test_box_query_host.py -- on the same arrays, bit for bit: box counts about the wave and block sizes, the counts alone, the exact
two-pass lists and fixed capacities, numpy and torch, box layouts, `visits` against the reference walk element for element, the entries no list
reaches left as they were, every node form (in fresh child processes), the dynamic mesh after a rebuild, a refit and a rebuild of parts (with
mesh_hit_parts over .hits(), and every list ascending on the device builders' trees), stream ordering with torch, isolation from the frame state, no
allocation after the first query, and the refusals.  The bodies are overlap_cases.py's, shared with the triangle and hull queries."""
import pytest

import box_query_ref as ref
import overlap_cases as oc
from query_gpu import _clean_env  # noqa: F401  (autouse)

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- 1: against the definition

@pytest.mark.parametrize("mesh", ref.MESHES)
def test_answers_equal_the_definition(mesh):
    oc.answers_equal_the_definition(oc.BOX, mesh)


def test_layouts_give_identical_bytes():
    oc.layouts_give_identical_bytes(oc.BOX)


def test_entries_no_list_reaches_are_left_as_they_were():
    """The C entries on arrays pre-filled with a sentinel, device and host path: the counts alone; lists alone in exact slots with a guard word behind;
    slots one short; fixed capacities; slots of negative length or with a negative start."""
    oc.entries_no_list_reaches_are_left_as_they_were(oc.BOX)


@pytest.mark.parametrize("option", ["RT_QNODES=2", "RT_FUSED=1", "RT_IMPLICIT=1"])
def test_every_node_form_gives_identical_bytes(option):
    """The query reads the two-child records and the triangle rows alone: what else the upload builds does not matter.  The options are read from
    the environment of the process, so each runs in a fresh child."""
    oc.every_node_form_gives_identical_bytes(oc.BOX, option)


# ---------------------------------------------------------------- 2: the dynamic mesh

def test_dynamic_mesh_rebuild_refit_and_parts():
    oc.dynamic_mesh_rebuild_refit_and_parts(oc.BOX)


# ---------------------------------------------------------------- 3: stream ordering with torch

def test_boxes_written_by_torch_just_before_the_call_are_the_ones_queried():
    oc.written_by_torch_just_before_the_call_are_the_ones_queried(oc.BOX)


def test_two_calls_on_two_torch_streams_without_a_host_wait():
    oc.two_calls_on_two_torch_streams_without_a_host_wait(oc.BOX)


# ---------------------------------------------------------------- 4: isolation from frames, no allocation

@pytest.mark.parametrize("pipeline", ["megakernel", "wavefront"])
def test_queries_do_not_touch_frame_state(pipeline):
    """Three BVH frames with box queries (host and device path) enqueued between them against the same three frames without: COLOR0 of every frame,
    the frame index, RtCounters (the megakernel's counting build), the traced-ray tallies and rt_debug_builds are identical."""
    oc.queries_do_not_touch_frame_state(oc.BOX, pipeline)


def test_no_allocation_after_the_first_query():
    oc.no_allocation_after_the_first_query(oc.BOX)


# ---------------------------------------------------------------- 5: refusals

def test_every_refusal_leaves_the_outputs_unwritten():
    oc.every_refusal_leaves_the_outputs_unwritten(oc.BOX)
