"""Action coverage (rmc_set_coverage; TLC's -coverage) without a device: the golden fixture
(tests/golden/coverage.json, tests/golden/make_golden_coverage.py) against the level fixtures of the same
configurations, its generator rerun on two small ones, and the launcher's usage errors."""
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import make_golden_coverage as MG  # noqa: E402

LAUNCHER = os.path.join(ROOT, "tla-raft_amd", "build", "raftmc")
VERDICTS = ("ok", "invariant", "assert", "eval_error", "deadlock")


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


COVERAGE = load("coverage.json")


def test_fixture_holds_the_twelve_configurations_and_every_verdict():
    assert list(COVERAGE) == list(MG.CONFIGS) and len(COVERAGE) == 12
    assert {e["verdict"] for e in COVERAGE.values()} == set(VERDICTS)
    assert {n: COVERAGE[n]["verdict"] for n in ("seeded_n3_v1_e2_r3", "sb_n3_v1_e2_r3", "deadlock_n3_v1_e1_r3",
                                                "cpl_n3_v2_e1_r3")} == {
        "seeded_n3_v1_e2_r3": "invariant", "sb_n3_v1_e2_r3": "assert", "deadlock_n3_v1_e1_r3": "deadlock",
        "cpl_n3_v2_e1_r3": "eval_error"}


@pytest.mark.parametrize("name", sorted(COVERAGE))
def test_sums_equal_the_level_fixture_totals(name):
    """1 + sum(generated) and 1 + sum(distinct) are TLC's two counters, in every outcome."""
    e = COVERAGE[name]
    g = load(e["levels_file"])[name]
    assert e["verdict"] == g["verdict"]
    assert len(e["generated"]) == len(e["distinct"]) == 13
    assert 1 + sum(e["generated"]) == e["total_generated"] == g["generated"]
    assert 1 + sum(e["distinct"]) == e["total_distinct"] == g["distinct"]
    assert all(d <= c for d, c in zip(e["distinct"], e["generated"]))
    assert e["generated"][11] == 0  # FollowerAppendEntry is never enabled
    if not name.startswith("bf_"):
        assert e["generated"][12] == 0


def test_per_level_arrays_are_cumulative_and_end_at_the_totals():
    e, g = COVERAGE["n3_v1_e1_r3"], load("levels.json")["n3_v1_e1_r3"]
    pl = e["per_level"]
    assert len(pl) == g["depth"]
    gen = [1 + sum(p["generated"]) for p in pl]
    dist = [1 + sum(p["distinct"]) for p in pl]
    assert [b - a for a, b in zip([1] + gen, gen)] == g["gen_per_level"]
    assert [b - a for a, b in zip([1] + dist, dist)][:-1] == g["levels"][1:] and dist[-1] == dist[-2]
    assert pl[-1] == dict(generated=e["generated"], distinct=e["distinct"])


def test_issue_findings():
    """What the fixture shows of the spec: BecomeFollower finds nothing new behind UpdateTerm, and
    FollowerRejectEntry never fires at MaxElection 1."""
    bf = COVERAGE["bf_n3_v1_e1_r3"]
    assert (bf["distinct"][12], bf["generated"][12], bf["generated"][1]) == (0, 148, 148)
    for n in ("n3_v1_e1_r3", "n4_v1_e1_r3", "n5_v1_e1_r3"):
        assert (COVERAGE[n]["distinct"][7], COVERAGE[n]["generated"][7]) == (0, 0)
    assert (COVERAGE["n2_v1_e2_r3"]["distinct"][7], COVERAGE["n2_v1_e2_r3"]["generated"][7]) == (26, 26)
    assert (COVERAGE["n3_v1_e2_r3"]["distinct"][7], COVERAGE["n3_v1_e2_r3"]["generated"][7]) == (7870, 12188)
    assert (COVERAGE["n3_v1_e2_r3"]["distinct"][6], COVERAGE["n3_v1_e2_r3"]["generated"][6]) == (50571, 485568)


@pytest.mark.parametrize("name", ["n3_v1_e1_r3", "sb_n3_v1_e2_r3"])
def test_generator_reproduces_the_committed_entry(name):
    got_name, e = MG.entry(name)
    assert got_name == name and e == COVERAGE[name]


@pytest.mark.parametrize("args,word", [
    (["-coverage"], "-coverage"),
    (["-coverage", "Raft.tla"], "-coverage"),
    (["-coverage", "1", "-simulate", "Raft.tla"], "-simulate"),
    (["-coverage", "1", "-recover", "states", "Raft.tla"], "-recover"),
])
def test_launcher_coverage_usage_errors(args, word):
    """Refused before any file is read or a device touched: TLC's -coverage needs its number of minutes,
    and neither a simulation nor a recovered run can report coverage."""
    r = subprocess.run([LAUNCHER] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 150, r.stdout + r.stderr
    assert "usage: raftmc" in r.stderr and word in r.stderr.splitlines()[0]
    assert r.stdout == ""
