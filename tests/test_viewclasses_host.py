"""CPU tests of the reference for counting the VIEW's classes among the states of a whole-state search
(tests/golden/viewclasses.json, make_golden_viewclasses.py: the Python oracle through tests/fullstate_ref.py):
the fixture against fullstate.json and against itself, the rooted runs in which the VIEW search misses classes,
and tools/view_gap.py's verdict on such counts.  No compute call is made here."""
import json
import os
import sys

import pytest

import fullstate_ref as F
import raft_ref as R
from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.join(GOLDEN))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden_viewclasses as M  # noqa: E402
import view_gap  # noqa: E402

FULL = json.load(open(os.path.join(GOLDEN, "fullstate.json")))
VC = json.load(open(os.path.join(GOLDEN, "viewclasses.json")))
RUNS = [("A/" + k, e) for k, e in sorted(VC["A"].items())] + [("B", VC["B"]), ("C", VC["C"])]
SMALL = "sym_n2_v1_e2_r2"


def test_run_a_is_fullstate_jsons_finished_two_server_runs():
    want = sorted(k for k, g in FULL.items() if g["verdict"] == "ok" and g["n"] == 2)
    assert sorted(VC["A"]) == want and len(want) == 5
    for name in want:
        g, e = FULL[name], VC["A"][name]
        assert e["classes"] == g["view_classes"] == g["view"]["distinct"], name
        assert e["states"] == g["distinct"] and e["levels"] == g["levels"], name
        # no class is hidden and each is met at its shortest depth: the firsts are the VIEW twin's levels
        assert e["class_levels"] == g["view"]["levels"], name


@pytest.mark.parametrize("name,e", RUNS, ids=[n for n, _ in RUNS])
def test_fixture_sums(name, e):
    h = e["size_hist"]
    assert len(h) == 32 and sum(h) == e["classes"] == sum(e["class_levels"])
    assert h[31] == 0 and sum((k + 1) * c for k, c in enumerate(h)) == e["states"] == sum(e["levels"])
    assert e["largest"] == max(k + 1 for k, c in enumerate(h) if c)
    assert len(e["class_levels"]) <= len(e["levels"])
    assert all(c <= s for c, s in zip(e["class_levels"], e["levels"]))
    assert 40 <= len(e["sample"]) <= 60
    assert all(1 <= s["members"] <= e["largest"] and 1 <= s["first_level"] <= len(e["levels"]) for s in e["sample"])
    assert any(s["members"] == e["largest"] for s in e["sample"])


def test_the_rooted_runs_have_the_gap():
    """B: [Init with restartCount = MaxRestart, Init].  The VIEW search keeps the spent copy and finds 327 of the
    1,061 classes; C: electionCount = MaxElection, 1 of them.  The whole-state search finds all, at Init's depths."""
    b, c, a = VC["B"], VC["C"], VC["A"][SMALL]
    assert (a["states"], a["classes"], a["size_hist"][:3]) == (1465, 1061, [657, 404, 0])
    assert (b["states"], b["generated"], b["classes"], b["size_hist"][:4]) == (1792, 3361, 1061, [552, 287, 222, 0])
    assert (b["view"]["distinct"], b["view"]["generated"], b["view"]["levels"][:8]) == (327, 581, [1, 1, 3, 4, 5, 7, 11, 19])
    assert b["class_levels"][:8] == [1, 1, 3, 4, 5, 8, 15, 30] and b["levels"][0] == 2
    assert (c["states"], c["generated"], c["classes"], c["size_hist"][:3]) == (1466, 2782, 1061, [656, 405, 0])
    assert (c["view"]["distinct"], c["view"]["generated"], c["view"]["levels"]) == (1, 2, [1])
    # both copies only raise a counter: every class Init reaches is reached, at its depth from Init
    assert b["class_levels"] == c["class_levels"] == a["class_levels"]
    for e in (b, c):
        assert len(e["roots"]) == 2 and e["roots"][1] == {**e["roots"][0], "restartCount": 0, "electionCount": 0}
        assert e["absent"]["commitIndex"] != e["roots"][1]["commitIndex"]


def test_generator_reproduces_the_smallest_run_and_run_c():
    """make_golden_viewclasses.py on the two quickest runs (a second or two each) gives the committed entries; its
    seeded search from Init alone is raft_ref.bfs under the whole-state identity."""
    name, e = M.run_a((SMALL, FULL[SMALL]))
    assert json.loads(json.dumps(e)) == VC["A"][SMALL]
    tag, e = M.run_roots("C")
    assert json.loads(json.dumps(e)) == VC["C"]
    cfg = R.Config(view=False, **M.SMALL)
    states, level, generated = M.seeded_bfs(cfg, [R.init_state(cfg)])
    r = F.bfs(cfg, keep_states=True)
    assert (len(states), generated, M.levels_of(level)) == (r.distinct, r.generated, r.levels)
    assert [F.whole(s) for s in states] == [F.whole(s) for s in r.states]


def _counts_dict(e, view):
    """A counting run's result in tools/view_gap.py's keys, held against a VIEW run of `view` (distinct, levels)."""
    a, b = view[1], e["class_levels"]
    diff = [i for i in range(max(len(a), len(b))) if (a[i] if i < len(a) else 0) != (b[i] if i < len(b) else 0)]
    return dict(view=(view[0], 0, 0), full=(e["states"], 0, 0), view_classes=e["classes"], streamed=e["states"],
                levels_agree=not diff, first_level_diff=diff[0] + 1 if diff else None)


def test_view_gap_verdict_for_a_gap_and_for_none():
    g = FULL[SMALL]
    none = _counts_dict(VC["A"][SMALL], (g["view"]["distinct"], g["view"]["levels"]))
    assert view_gap.verdict(none) == "the VIEW run missed no class" and none["levels_agree"]
    b = VC["B"]
    gap = _counts_dict(b, (b["view"]["distinct"], b["view"]["levels"]))
    assert view_gap.verdict(gap) == "the VIEW hid 734 classes"
    assert (gap["levels_agree"], gap["first_level_diff"]) == (False, 6)
    cut = dict(gap, stopped="RMC_E_MEMORY: hipMalloc", streamed=900)
    assert view_gap.verdict(cut).startswith("not decided: 900 of 1,792 states")
