"""Continuation (rmc_set_continue; TLC's -continue) without a device: the golden fixture
(tests/golden/continue.json, tests/golden/make_golden_continue.py) against itself and against the level
fixtures of the same configurations, its generator rerun on the small entries, the new exports and the
launcher's argument handling."""
import json
import os
import subprocess
import sys

import pytest

import raftmc
from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import make_golden_continue as MG  # noqa: E402

LAUNCHER = os.path.join(ROOT, "tla-raft_amd", "build", "raftmc")


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


CONT = load("continue.json")


def test_fixture_holds_the_ten_entries_and_the_issue_spot_values():
    # (the issue's ten entries, then cpl_nac_n3_v2_e1_r3, which has no spot values)
    assert list(CONT) == list(MG.CONFIGS) and list(CONT)[:10] == list(MG.SPOT) and len(CONT) == 11
    for name, (head, per_inv) in MG.SPOT.items():
        e = CONT[name]
        assert (e["verdict"], e["generated"], e["distinct"], e["depth"]) == head, name
        assert list(e["violations"]) == e["invariants"] == list(per_inv), name
        for nm, want in per_inv.items():
            v = e["violations"][nm]
            assert (v["count"], v["first_gid"], v["first_level"]) == want, (name, nm)
    assert {e["verdict"] for e in CONT.values()} == {"ok", "assert", "eval_error", "deadlock"}


@pytest.mark.parametrize("name", list(CONT))
def test_fixture_is_self_consistent(name):
    e = CONT[name]
    total = 0
    for nm, v in e["violations"].items():
        assert len(v["per_level"]) == e["depth"] and sum(v["per_level"]) == v["count"], nm
        total += v["count"]
        if v["count"] == 0:
            assert v["first_gid"] is None and v["first_level"] is None and v["first_path"] is None
            continue
        # the first state lies in the first level that holds a violation, and its path has a step per level
        assert v["first_level"] == 1 + next(i for i, c in enumerate(v["per_level"]) if c)
        assert len(v["first_path"]) == v["first_level"] - 1
        assert 0 <= v["first_gid"] < e["distinct"]
        assert (v["first_gid"] == 0) == (v["first_level"] == 1)
    assert total <= e["distinct"]  # a state is attributed to one invariant
    if "coverage" in e:
        assert 1 + sum(e["coverage"]["generated"]) == e["generated"]
        assert 1 + sum(e["coverage"]["distinct"]) == e["distinct"]


@pytest.mark.parametrize("name", [n for n, e in CONT.items() if e["levels_file"]])
def test_exhausted_entries_have_the_counters_of_the_run_without_violations(name):
    """A run that goes on past every violation explores what the configuration's full exhaustion explores."""
    e = CONT[name]
    g = load(e["levels_file"])[e["levels_key"]]
    assert e["verdict"] == g["verdict"] == "ok"
    assert (e["generated"], e["distinct"], e["depth"]) == (g["generated"], g["distinct"], g["depth"])


def test_stopping_entries_stop_where_the_error_fixtures_stop():
    le, lv = load("levels_errors.json"), load("levels.json")
    for name, g in (("cpl_n3_v2_e1_r3", le["cpl_n3_v2_e1_r3"]), ("deadlock_n3_v1_e1_r3", lv["deadlock_n3_v1_e1_r3"])):
        e = CONT[name]
        assert (e["verdict"], e["generated"], e["distinct"], e["depth"]) == \
            (g["verdict"], g["generated"], g["distinct"], g["depth"])
    # the stop-at-first-violation run of the split-brain entry ends at its first NoSplitVote state; this one
    # goes on to the Assert
    g, e = le["sb_n3_v1_e3_r3"], CONT["sb_n3_v1_e3_r3"]
    assert g["verdict"] == "invariant" and g["violated"] == "NoSplitVote"
    assert e["violations"]["NoSplitVote"]["first_gid"] == g["distinct"] - 1 == 55
    assert e["violations"]["NoSplitVote"]["first_level"] == g["depth"]
    # ... and the seeded bug's first Inv violation is the state levels.json stops at
    g, e = lv["seeded_n3_v1_e2_r3"], CONT["seeded_n3_v1_e2_r3"]
    assert e["violations"]["Inv"]["first_gid"] == g["distinct"] - 1 == 3455
    assert e["violations"]["Inv"]["first_level"] == g["depth"] == len(e["violations"]["Inv"]["first_path"]) + 1


@pytest.mark.parametrize("name", ["n2_v1_e2_r3", "bf_n3_v1_e1_r3", "sb_n3_v1_e3_r3", "cpl_n3_v2_e1_r3",
                                  "deadlock_n3_v1_e1_r3", "cpl_nac_n3_v2_e1_r3"])
def test_generator_reproduces_the_committed_entry(name):
    got_name, e = MG.entry(name)
    assert got_name == name and json.loads(json.dumps(e)) == CONT[name]


def test_library_exports_the_continuation_entry_points():
    lib = raftmc.load_library()
    for sym in ("rmc_set_continue", "rmc_get_violations", "rmc_get_violation_levels", "rmc_violation_trace"):
        assert hasattr(lib, sym), sym
    for method in ("set_continue", "violations", "violation_levels", "violation_trace"):
        assert callable(getattr(raftmc.ModelChecker, method, None)), method
    assert lib.rmc_abi_version() == 5


@pytest.mark.parametrize("args,word", [
    (["-continue", "-simulate", "Raft.tla"], "-simulate"),
    (["-simulate", "num=10", "-continue", "Raft.tla"], "-simulate"),
    (["-continue", "-recover", "states", "Raft.tla"], "-recover"),
])
def test_launcher_continue_usage_errors(args, word):
    """Refused before any file is read or a device touched: a simulation stops at its first error, and
    checkpoints do not carry the violation counts."""
    r = subprocess.run([LAUNCHER] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 150, r.stdout + r.stderr
    first = r.stderr.splitlines()[0]
    assert "usage: raftmc" in r.stderr and "-continue" in first and word in first
    assert r.stdout == ""


def test_launcher_takes_continue(tmp_path):
    """-continue is an option now: without a model the run fails like any other (no spec file), with one
    and no device at device creation -- never as an unsupported option."""
    r = subprocess.run([LAUNCHER, "-continue"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 150 and "missing spec file" in r.stderr and "unsupported option" not in r.stderr
    from conftest import has_gpu
    if has_gpu():
        return
    from test_host import cfg_text
    (tmp_path / "Raft.cfg").write_text(cfg_text(E=1, R=3, vals="v1"))
    r = subprocess.run([LAUNCHER, "-continue", "-deadlock", "-config", str(tmp_path / "Raft.cfg"),
                        str(tmp_path / "Raft.tla")], capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, RMC_SKIP_SPEC_CHECK="1"))
    assert "unsupported option" not in r.stderr and "usage: raftmc" not in r.stderr
    assert r.returncode == 75 and "could not start the GPU model checker" in r.stdout
