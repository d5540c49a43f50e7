"""The expected-value helper of the mutation-layer decode tests, held to the
reference's own known answers and to hand-written literals (CPU only).

rows_mut_ref.want_row is a set expression: sorted((P - uids(M)) | sets(M)),
then x > after, then first.  tests/golden/mutation_layer.json holds what the
reference's posting/list_test.go expects of List.Uids and List.Length on lists
with a mutable layer, as data.
"""
import json
import os

import gv_spec as gv
import rows_decode_ref
from rows_mut_ref import MUT_DEL, MUT_OVR, MUT_SET, flat, want_row, want_rows

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "mutation_layer.json")


def golden_cases():
    for c in json.load(open(GOLDEN))["cases"]:
        pack = list(range(*c["pack_range"])) if "pack_range" in c else c["pack"]
        newest = {}
        for start, stop, step, op in c.get("mut_ranges", []):
            for u in range(start, stop, step):
                newest[u] = op
        for u, op in c.get("muts", []):
            newest[u] = op
        yield c, pack, sorted(newest.items())


def test_reference_known_answers():
    names = set()
    for c, pack, muts in golden_cases():
        got = want_row(pack, muts, c["after"])
        if "want" in c:
            assert got == c["want"], c["name"]
        else:
            assert len(got) == c["want_len"], c["name"]
        names.add(c["name"].split("/")[0])
    assert {"TestAddMutation", "TestAddMutation_DelSet", "TestAddMutation_DelRead",
            "TestAddAndDelMutation", "TestDelete", "TestListDeleteMarker",
            "TestAfterUIDCount"} <= names


def test_empty_layer_is_the_plain_decode():
    uids = gv.seek_pack()
    for a in gv.seek_list(gv.encode(uids, 9)):
        for f in (0, 1, -1, 9, -10, 2**31 - 1, -2**31):
            assert want_row(uids, [], a, f) == rows_decode_ref.want_row(uids, a, f)
    u = [3, 5, 8, 13, 21]
    assert want_rows([u, [], [0, 7]], [[], [], []], [5, 0, 0], [-2, 1, -1]) == \
        rows_decode_ref.want_rows([u, [], [0, 7]], [5, 0, 0], [-2, 1, -1])


def test_rule_1_merge_literals():
    p = [3, 5, 8, 13, 21]
    assert want_row(p, [(4, MUT_SET)]) == [3, 4, 5, 8, 13, 21]
    assert want_row(p, [(5, MUT_SET)]) == p                 # present: emitted once
    assert want_row(p, [(5, MUT_DEL)]) == [3, 8, 13, 21]
    assert want_row(p, [(6, MUT_DEL)]) == p                 # absent: nothing happens
    assert want_row(p, [(5, MUT_OVR)]) == p                 # any op but Del sets
    assert want_row(p, [(6, MUT_OVR), (7, 0), (9, 255)]) == [3, 5, 6, 7, 8, 9, 13, 21]
    assert want_row(p, [(1, MUT_SET), (3, MUT_DEL), (21, MUT_DEL), (22, MUT_SET)]) == \
        [1, 5, 8, 13, 22]
    assert want_row([], [(2, MUT_SET), (7, MUT_DEL), (9, MUT_SET)]) == [2, 9]
    assert want_row([], [(7, MUT_DEL)]) == []
    assert want_row(p, [(u, MUT_DEL) for u in p]) == []
    assert want_row(p, [(gv.U64_MAX, MUT_SET)]) == p + [gv.U64_MAX]


def test_rule_2_after_is_strict_on_both_sides():
    p = [3, 5, 8, 13, 21]
    m = [(4, MUT_SET), (8, MUT_DEL), (9, MUT_SET), (30, MUT_SET)]
    assert want_row(p, m) == [3, 4, 5, 9, 13, 21, 30]
    assert want_row(p, m, 4) == [5, 9, 13, 21, 30]          # a set uid: dropped itself
    assert want_row(p, m, 8) == [9, 13, 21, 30]             # a deleted uid
    assert want_row(p, m, 5) == [9, 13, 21, 30]             # a pack uid
    assert want_row(p, m, 29) == [30] and want_row(p, m, 30) == []
    assert want_row(p, m, 1) == want_row(p, m, 0)
    assert want_row(p, m, gv.U64_MAX) == []


def test_rule_3_and_4_first_and_defaults():
    p = [3, 5, 8, 13, 21]
    m = [(4, MUT_SET), (8, MUT_DEL), (9, MUT_SET), (30, MUT_SET)]
    assert want_row(p, m, 0, 2) == [3, 4]                   # the edge on a set
    assert want_row(p, m, 0, 1) == [3] and want_row(p, m, 0, -1) == [30]
    assert want_row(p, m, 0, -3) == [13, 21, 30]
    assert want_row(p, m, 4, 2) == [5, 9] and want_row(p, m, 4, -2) == [21, 30]
    assert want_row(p, m, 0, 2**31 - 1) == want_row(p, m, 0, -2**31) == want_row(p, m)
    assert want_rows([p, []], [m, [(1, MUT_SET)]]) == [want_row(p, m), [1]]
    assert flat([m, [], [(1, MUT_SET)]]) == ([4, 8, 9, 30, 1], [1, 2, 1, 1, 1], [0, 4, 4, 5])
