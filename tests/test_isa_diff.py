"""tools/isa_diff.py pairs the symbols that left a code object: renamed (same code object, another name, identical code) and moved (another code
object, the same name, identical code).  Only a symbol with no such partner counts as removed."""
import importlib.util
from pathlib import Path

_spec = importlib.util.spec_from_file_location("isa_diff", Path(__file__).resolve().parent.parent / "tools" / "isa_diff.py")
isa_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_diff)

BODY = ["s_load_dword s0, s[4:5], 0x0", "s_cbranch_scc1 8 // <k_a+0x40>", "s_endpgm"]


def test_a_kernel_in_another_code_object_with_identical_code_has_moved():
    before = {(6, "k_a"): BODY, (6, "k_b"): BODY[:2], (6, "k_c"): BODY}
    after = {(17, "k_a"): list(BODY), (18, "k_b"): BODY[:1], (17, "k_new"): BODY}
    gone = [k for k in before if k not in after]
    added = [k for k in after if k not in before]
    gone, added, moved = isa_diff.pair_moved(before, after, gone, added)
    assert moved == [((6, "k_a"), (17, "k_a"))]
    assert gone == [(6, "k_b"), (6, "k_c")]                          # k_b's code changed on the way, k_c has no namesake: both still count as removed
    assert added == [(18, "k_b"), (17, "k_new")]


def test_a_rename_stays_inside_its_code_object():
    before = {(6, "k_a"): BODY}
    after = {(6, "k_z"): [line.replace("k_a", "k_z") for line in BODY], (7, "k_y"): BODY}
    gone, added, renamed = isa_diff.pair_renamed(before, after, [(6, "k_a")], [(6, "k_z"), (7, "k_y")])
    assert renamed == [((6, "k_a"), (6, "k_z"))] and gone == [] and added == [(7, "k_y")]
