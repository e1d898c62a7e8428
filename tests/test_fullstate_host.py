"""CPU tests of the whole-state search (rmc_set_full_state, ModelConfig(view=False), raftmc -fullstate):
the reference and its fixture (tests/fullstate_ref.py, tests/golden/fullstate.json), the C interface, the
launcher's argument handling and tools/view_gap.py's counting.  No compute call is made here."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fullstate_ref as F
import raft_ref as R
import raftmc
from conftest import GOLDEN, ROOT, has_gpu
from test_host import HEADER, LAUNCHER, cfg_text

sys.path.insert(0, os.path.join(ROOT, "tools"))
import view_gap  # noqa: E402

FULL = json.load(open(os.path.join(GOLDEN, "fullstate.json")))
LEVELS = json.load(open(os.path.join(GOLDEN, "levels.json")))
SMALL = "sym_n2_v1_e2_r2"


def ref_cfg(g, view):
    return R.Config(n=g["n"], V=g["V"], max_election=g["E"], max_restart=g["R"], seeded=g["seeded"],
                    become_follower=g["become_follower"], symmetry=g["symmetry"], invariants=tuple(g["invariants"]),
                    check_deadlock=g["check_deadlock"], view=view)


def test_fixture_holds_the_configurations_and_every_entry_differs_from_its_view_twin():
    assert {"sym_n2_v1_e2_r2", "sym_n2_v2_e2_r2", "nosym_n2_v1_e2_r2", "nosym_n2_v2_e2_r2", "sym_n3_v1_e2_r1",
            "seeded_n3_v1_e2_r1"} <= set(FULL)
    assert sum(k.startswith("deadlock_") for k in FULL) == 1 and sum(k.startswith("bf_") for k in FULL) == 1
    assert len(FULL) == 8
    for name, g in FULL.items():
        v = g["view"]
        assert (g["generated"], g["distinct"], g["levels"]) != (v["generated"], v["distinct"], v["levels"]), name
        assert g["distinct"] >= v["distinct"], name
        if g["verdict"] == "ok":
            # every state a VIEW run keeps is reachable: the whole-state run meets at least its classes
            assert v["distinct"] <= g["view_classes"] <= g["distinct"], name
    assert FULL["seeded_n3_v1_e2_r1"]["verdict"] == "invariant" and FULL["seeded_n3_v1_e2_r1"]["trace_len"] == 12
    assert next(g for k, g in FULL.items() if k.startswith("deadlock_"))["verdict"] == "deadlock"
    assert next(g for k, g in FULL.items() if k.startswith("bf_"))["become_follower"]


# the entries the Python reference finishes in a second or two each (the 2-value and the exhausted 3-server rows
# take from ten seconds to minutes: their VIEW twins are held to levels.json below where it has them)
QUICK = sorted(k for k, g in FULL.items() if g["distinct"] < 5000)


def test_quick_rows_are_most_of_the_fixture():
    assert len(QUICK) >= 5 and SMALL in QUICK and any(FULL[k]["verdict"] == "invariant" for k in QUICK)
    assert any(FULL[k]["verdict"] == "deadlock" for k in QUICK) and any(FULL[k]["become_follower"] for k in QUICK)


@pytest.mark.parametrize("name", QUICK)
def test_reference_reproduces_the_view_run_and_the_fixture(name):
    """raft_ref.bfs unchanged gives the fixture's VIEW twin; fullstate_ref.bfs the whole-state entry (counters at
    an error and the counterexample included), and the view-class count comes from its states."""
    g = FULL[name]
    rv = R.bfs(ref_cfg(g, True))
    v = g["view"]
    assert (rv.verdict, rv.distinct, rv.generated, rv.depth, rv.levels, rv.queue_left) == (
        v["verdict"], v["distinct"], v["generated"], v["depth"], v["levels"], v["queue_left"])
    rf = F.bfs(ref_cfg(g, False), keep_states=True)
    assert (rf.verdict, rf.distinct, rf.generated, rf.depth, rf.levels, rf.generated_per_level, rf.queue_left) == (
        g["verdict"], g["distinct"], g["generated"], g["depth"], g["levels"], g["gen_per_level"], g["queue_left"])
    if rf.trace:
        assert [(list(k) if k else None, R.state_to_json(st)) for k, st in rf.trace] == \
            [(e["key"], e["state"]) for e in g["steps"]]
    if g["verdict"] == "ok":
        assert F.view_classes(ref_cfg(g, False), rf.states) == g["view_classes"]
    assert R.canonical is not F.canonical  # (the wrapper put raft_ref's own identity back)


def test_view_twins_equal_levels_json_where_they_overlap():
    hit = 0
    for name, g in FULL.items():
        key = f"n{g['n']}_v{g['V']}_e{g['E']}_r{g['R']}"
        if key in LEVELS and g["symmetry"] and not (g["seeded"] or g["become_follower"] or g["check_deadlock"]):
            lv = LEVELS[key]
            assert (g["view"]["distinct"], g["view"]["generated"], g["view"]["levels"]) == (
                lv["distinct"], lv["generated"], lv["levels"]), name
            hit += 1
    assert hit >= 1


def test_whole_state_identity_is_a_symmetry_class_invariant():
    """fullstate_ref.canonical: a permuted copy (hidden variables permuted with the rest) has the state's
    identity; a copy with one hidden component changed has another; the VIEW identity sees neither change."""
    cfg = R.Config(n=3, V=1, max_election=2, max_restart=2, view=False)
    vcfg = R.Config(n=3, V=1, max_election=2, max_restart=2)
    r = F.bfs(R.Config(n=3, V=1, max_election=1, max_restart=1, view=False), keep_states=True)
    for st in r.states[::97]:
        base = F.canonical(cfg, st)
        for pi in ((1, 0, 2), (2, 0, 1)):
            assert F.canonical(cfg, F.permute_state(st, pi)) == base
        seen = {base}
        for label, cp in F.hidden_copies(st):
            c = F.canonical(cfg, cp)
            assert R.canonical(vcfg, cp) == R.canonical(vcfg, st), label
            assert F.whole(cp) != F.whole(st), label
            seen.add(c)
        assert len(seen) > 1


def test_library_exports_the_setter_and_abi_stays_5():
    lib = raftmc.load_library()
    assert hasattr(lib, "rmc_set_full_state")
    text = open(HEADER).read()
    assert re.search(r"^int rmc_set_full_state\(void \*ctx, int on\);", text, re.M)
    assert "#define RMC_ABI_VERSION 5" in text and lib.rmc_abi_version() == 5
    assert "is always on" not in text
    assert raftmc.ModelConfig().view is True and hasattr(raftmc.ModelChecker, "set_full_state")


def test_cfg_without_the_view_line_is_still_refused_and_names_the_flag():
    with pytest.raises(raftmc.RmcError, match="VIEW") as e:
        raftmc.parse_config(cfg_text().replace("VIEW view", ""))
    assert "-fullstate" in str(e.value)


def test_launcher_refuses_fullstate_with_simulate(tmp_path):
    (tmp_path / "Raft.cfg").write_text(cfg_text(E=2, R=2, servers="s1, s2", vals="v1"))
    env = dict(os.environ, RMC_SKIP_SPEC_CHECK="1")
    r = subprocess.run([LAUNCHER, "-fullstate", "-simulate", "num=10", "-config", str(tmp_path / "Raft.cfg"),
                        str(tmp_path / "Raft.tla")], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 150 and "-fullstate cannot be combined with -simulate" in r.stderr
    assert "Starting" not in r.stdout  # refused before the header, so before a device is opened


def test_launcher_accepts_fullstate(tmp_path):
    """-fullstate is parsed, the header carries the new line; without a GPU the run ends at the device error."""
    g = FULL[SMALL]
    (tmp_path / "Raft.cfg").write_text(cfg_text(E=g["E"], R=g["R"], servers="s1, s2", vals="v1"))
    env = dict(os.environ, RMC_SKIP_SPEC_CHECK="1")
    r = subprocess.run([LAUNCHER, "-fullstate", "-deadlock", "-config", str(tmp_path / "Raft.cfg"),
                        str(tmp_path / "Raft.tla")], capture_output=True, text=True, env=env, timeout=120)
    out = r.stdout.splitlines()
    k = next(i for i, ln in enumerate(out) if ln.startswith("Starting... ("))
    assert out[k + 1] == "Fingerprinting the whole state: the cfg's VIEW view is not applied."
    if has_gpu():
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"{g['generated']} states generated, {g['distinct']} distinct states found" in r.stdout
    else:
        assert r.returncode == 75, r.stdout + r.stderr
        assert sum(ln.startswith("Error: could not start the GPU model checker") for ln in out) == 1
    usage = subprocess.run([LAUNCHER, "-bogus", "Raft.tla"], capture_output=True, text=True).stderr
    assert "-fullstate" in usage
    assert "-fullstate" in open(os.path.join(ROOT, "tla-raft_amd", "myrun.sh")).read()


def _digest_fps(cfg, states):
    """A stand-in for the VIEW checker's fingerprints: 128 bits of a digest of the reference's VIEW identity."""
    out = np.empty((len(states), 2), dtype=np.uint64)
    for i, st in enumerate(states):
        d = hashlib.sha256(repr(R.canonical(cfg, st)).encode()).digest()
        out[i] = (int.from_bytes(d[:8], "little"), int.from_bytes(d[8:16], "little"))
    return out


@pytest.mark.parametrize("name", [SMALL, "nosym_n2_v1_e2_r2"])
def test_view_gap_counting_on_the_reference_states(name):
    """tools/view_gap.py's ClassCounter over the reference's whole-state run, chunk by chunk, gives the fixture's
    view-class count, whatever the chunking."""
    g = FULL[name]
    r = F.bfs(ref_cfg(g, False), keep_states=True)
    fps = _digest_fps(ref_cfg(g, True), r.states)
    for chunk in (7, 256, len(fps)):
        c = view_gap.ClassCounter()
        for a in range(0, len(fps), chunk):
            c.add(fps[a:a + chunk])
        assert c.total == g["distinct"] and c.count() == g["view_classes"], chunk
    assert view_gap.verdict(dict(view_classes=g["view_classes"], view=(g["view"]["distinct"], 0, 0))) == \
        "the VIEW run missed no class"
    assert view_gap.verdict(dict(view_classes=5, view=(3, 0, 0))) == "the VIEW hid 2 classes"


def test_class_counter_edge_cases():
    c = view_gap.ClassCounter()
    assert c.count() == 0
    c.add(np.array([[1, 2]], dtype=np.uint64))
    c.add(np.array([[1, 3], [2, 2], [1, 2]], dtype=np.uint64))  # equal x or equal y alone is not equality
    c.add(np.zeros((0, 2), dtype=np.uint64))
    assert c.count() == 3 and c.total == 4
