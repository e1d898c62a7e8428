"""Continuation on the GPU (rmc_set_continue / rmc_get_violations; raftmc -continue): the search goes on
past invariant violations and counts them per invariant, against tests/golden/continue.json (the Python
oracle, tests/golden/make_golden_continue.py).  Integers: every comparison is exact.

Every execution path counts: the device-driven level loop (a scan launch behind each level's commit, rows per
level on the device), host-driven fused levels and chunks, split chunks with look-ahead, virtual shards with and without replicated levels, the
one-rank RCCL communicator and two rank processes over the host transport.  The three stopping entries
(Assert, evaluation error, deadlock) are the ones a level-wide count -- one that does not cut at TLC's
stopping point -- would fail."""
import json
import os
import re
import socket
import subprocess
import sys

import pytest

import raftmc
from conftest import GOLDEN
from test_gpu import check_levels, spec_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


CONT = load("continue.json")
# (cpl_nac_n3_v2_e1_r3: the counted invariant, NoAllCommit, reads the records' message ids -- at the cut of a
# sharded round from the outbox)
STOPPING = ["sb_n3_v1_e3_r3", "cpl_n3_v2_e1_r3", "deadlock_n3_v1_e1_r3", "cpl_nac_n3_v2_e1_r3"]
STATUS = {"ok": "done"}


def cfg_kw(name, **kw):
    c = CONT[name]["config"]
    variant = raftmc.SPEC_RAFT
    if c.get("become_follower"):
        variant = raftmc.SPEC_BECOME_FOLLOWER
    elif c.get("split_brain"):
        variant = raftmc.SPEC_SPLIT_BRAIN
    elif c.get("commit_past_log"):
        variant = raftmc.SPEC_COMMIT_PAST_LOG
    elif c.get("seeded"):
        variant = raftmc.SPEC_SEEDED
    return dict(n_servers=c["n"], n_vals=c["V"], max_election=c["max_election"], max_restart=3,
                invariants=tuple(c["invariants"]), check_deadlock=bool(c.get("check_deadlock")), spec_variant=variant,
                **kw)


def make(name, **kw):
    return raftmc.ModelChecker(raftmc.ModelConfig(**cfg_kw(name, **kw)))


def expected(name):
    return {nm: (v["count"], v["first_level"]) for nm, v in CONT[name]["violations"].items()}


def check_run(name, mc, res):
    """Counters, verdict, violations(), violation_levels() and the first states' levels against the fixture."""
    e = CONT[name]
    assert res.status == STATUS.get(e["verdict"], e["verdict"])
    assert (res.generated, res.distinct, res.depth) == (e["generated"], e["distinct"], e["depth"])
    # (the only compiled invariant that can raise is Inv: logs[p][index], tla:499)
    assert res.violated == ("Inv" if e["verdict"] == "eval_error" else None)
    got = mc.violations()
    assert list(got) == e["invariants"]
    assert got == expected(name)
    for nm, v in e["violations"].items():
        assert mc.violation_levels(nm) == v["per_level"], nm


def check_traces(name, mc):
    for nm, v in CONT[name]["violations"].items():
        if not v["count"]:
            with pytest.raises(raftmc.RmcError, match="RMC_E_ARG"):
                mc.violation_trace(nm)
            continue
        tr = mc.violation_trace(nm)
        assert tr[0][0] is None and [list(k) for k, _ in tr[1:]] == v["first_path"], nm
        assert mc.eval_invariant(tr[-1][1], nm) is False, nm
        # ... and no invariant listed before it fails there: the state is attributed to the first FALSE one
        for before in CONT[name]["invariants"][:CONT[name]["invariants"].index(nm)]:
            assert mc.eval_invariant(tr[-1][1], before) is True, (nm, before)


def run_continued(name, traces=False, **kw):
    with make(name, **kw) as mc:
        mc.set_continue()
        res = mc.run()
        check_run(name, mc, res)
        if traces:
            check_traces(name, mc)
        return mc.violations()


# ---- 1. default settings ---------------------------------------------------------------------------------
def test_fixture_covers_the_kernel_variants():
    cs = [e["config"] for e in CONT.values()]
    assert {c["n"] for c in cs} == {2, 3, 4} and {c["V"] for c in cs} == {1, 2}
    assert any(c.get("become_follower") for c in cs) and all(n in CONT for n in STOPPING)
    assert "NoAllCommit" in CONT["n4_v1_e1_r3"]["invariants"]  # reads msgs, 128 message lanes


@pytest.mark.parametrize("name", list(CONT))
def test_violations_match_golden_default_settings(name):
    run_continued(name, traces=True)


# ---- 2. levels per host round trip ------------------------------------------------------------------------
@pytest.mark.parametrize("device_levels", [0, 1, 4])
@pytest.mark.parametrize("name", ["n2_v1_e2_r3", "sb_n3_v1_e3_r3"])
def test_violations_do_not_depend_on_device_levels(name, device_levels):
    run_continued(name, traces=True, device_levels=device_levels)


@pytest.mark.parametrize("name", ["n2_v1_e2_r3", "sb_n3_v1_e3_r3", "cpl_nac_n3_v2_e1_r3"])
def test_the_device_loop_runs_with_continuation_on(name):
    """Several levels per host round trip (rmc_steps) while the violations are counted: the loop neither steps
    aside, nor stops at a violation, nor miscuts at the error that ends it."""
    e = CONT[name]
    with make(name, device_levels=4) as mc:
        mc.set_continue()
        mc.init()
        trips = []
        while True:
            out = mc.steps()
            trips.append(len(out))
            # between round trips the counts stand at a level boundary
            if out[-1].status == "ok":
                lvl = out[-1].level + 1
                for nm, v in e["violations"].items():
                    assert mc.violation_levels(nm) == v["per_level"][:lvl], (lvl, nm)
            else:
                break
        assert max(trips) == 4, trips
        check_run(name, mc, mc.result())
        check_traces(name, mc)


def test_violations_after_every_level():
    """Between steps the counts cover the levels finished so far."""
    name = "n2_v1_e2_r3"
    e = CONT[name]
    with make(name, device_levels=1) as mc:
        mc.set_continue()
        mc.init()
        for lvl in range(1, e["depth"] + 1):
            got = mc.violations()
            for nm, v in e["violations"].items():
                part = v["per_level"][:lvl]
                first = v["first_level"] if v["first_level"] and v["first_level"] <= lvl else None
                assert got[nm] == (sum(part), first), (lvl, nm)
                assert mc.violation_levels(nm) == part, (lvl, nm)
            ls = mc.step()
        assert ls.status == "done"


# ---- 3. split chunks with look-ahead ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n3_v1_e2_r3", "n3_v1_e2_r3_b", "n4_v1_e1_r3", "seeded_n3_v1_e2_r3",
                                  "cpl_n3_v2_e1_r3"])
def test_violations_split_chunks_with_lookahead(name, monkeypatch):
    monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    run_continued(name, traces=True, device_levels=1, chunk_successors=6000)


# ---- 4. sharded --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [2, 3])
@pytest.mark.parametrize("name", ["n3_v1_e2_r3", "sb_n3_v1_e3_r3", "cpl_n3_v2_e1_r3"])
def test_violations_virtual_shards(name, shards):
    run_continued(name, traces=True, virtual_shards=shards, chunk_successors=3000, shard_min_states=1)


def test_violations_count_replicated_levels_once():
    run_continued("n2_v1_e2_r3", traces=True, virtual_shards=2, chunk_successors=3000, shard_min_states=40)


def test_violations_one_rank_rccl():
    run_continued("n3_v1_e2_r3", traces=True, world_size=1, rank=0, comm_unique_id=raftmc.comm_unique_id(),
                  chunk_successors=3000, shard_min_states=1)


@pytest.mark.parametrize("name", ["n2_v1_e2_r3", "sb_n3_v1_e3_r3"])
def test_violations_two_rank_processes_over_the_host_transport(name, tmp_path):
    """Each rank counts its part of every level; the all-reduces sum the counts and take the smallest first
    state, so both ranks report the global totals."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cfg = cfg_kw(name, chunk_successors=3000, shard_min_states=1)
    cfg["invariants"] = list(cfg["invariants"])
    procs, outs = [], []
    for r in range(2):
        outs.append(str(tmp_path / f"rank{r}.json"))
        spec = dict(rank=r, world=2, port=port, cfg=cfg, out=outs[-1])
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "continue_worker.py"), json.dumps(spec)],
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                                      env=dict(os.environ, RMC_COLL_CHECK="1")))
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=180)[0])
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
        for p in procs:
            p.wait()
        raise AssertionError("a rank did not finish (left in a collective?)")
    for p, log in zip(procs, logs):
        assert p.returncode == 0, log[-3000:]
    e = CONT[name]
    for o in outs:
        with open(o) as f:
            r = json.load(f)
        assert "error" not in r, r.get("error")
        assert (r["status"], r["generated"], r["distinct"], r["depth"]) == \
            (STATUS.get(e["verdict"], e["verdict"]), e["generated"], e["distinct"], e["depth"])
        assert {k: tuple(v) for k, v in r["violations"].items()} == expected(name)
        assert r["levels"] == {nm: v["per_level"] for nm, v in e["violations"].items()}
        assert r["paths"] == {nm: v["first_path"] for nm, v in e["violations"].items() if v["count"]}


# ---- 5. the cut at a stopping error -------------------------------------------------------------------------
PATHS = {
    "fused": dict(),
    "host_chunks": dict(device_levels=1, chunk_successors=3000),
    "split": dict(device_levels=1, chunk_successors=6000),
    "shards2": dict(virtual_shards=2, chunk_successors=3000, shard_min_states=1),
    "shards3_replicated_first": dict(virtual_shards=3, chunk_successors=3000, shard_min_states=30),
    "rccl1": dict(world_size=1, rank=0, chunk_successors=3000, shard_min_states=1),
}


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", STOPPING)
def test_nothing_beyond_the_cut_is_counted(name, path, monkeypatch):
    """The erring level holds violating states that TLC -workers 1 never reaches -- by the oracle, 9 more
    NoSplitVote states in sb_n3_v1_e3_r3's level 7 and 59 more RaftCanCommt states in cpl_n3_v2_e1_r3's level
    17 (none in deadlock_n3_v1_e1_r3, whose deadlocked parent is its level's last with new successors) -- so a
    count of the whole level fails here: the counts equal the oracle's, which stops there."""
    if path == "split":
        monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    kw = dict(PATHS[path])
    if path == "rccl1":
        kw["comm_unique_id"] = raftmc.comm_unique_id()
    got = run_continued(name, **kw)
    assert sum(c for c, _ in got.values()) <= CONT[name]["distinct"]


# ---- 6. lifecycle ------------------------------------------------------------------------------------------
def test_continuation_is_off_by_default():
    """... and with it off the same configurations stop where the level fixtures say."""
    for lv, key, name in (("levels.json", "seeded_n3_v1_e2_r3", "seeded_n3_v1_e2_r3"),
                          ("levels_errors.json", "sb_n3_v1_e3_r3", "sb_n3_v1_e3_r3")):
        g = load(lv)[key]
        kw = cfg_kw(name)
        kw["invariants"] = tuple(g["invariants"])
        assert kw["spec_variant"] == spec_of(g)
        with raftmc.ModelChecker(raftmc.ModelConfig(**kw)) as mc:
            res = mc.run()
            check_levels(g, res)
            assert res.status == "invariant"
            for call in (mc.violations, lambda: mc.violation_levels(g["violated"]), lambda: mc.violation_trace(g["violated"])):
                with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
                    call()


def test_the_fixture_invariant_lists_stop_without_continuation():
    """sb_n3_v1_e3_r3 with the fixture's own list (Inv, NoSplitVote) and continuation off: 56 states."""
    g = load("levels_errors.json")["sb_n3_v1_e3_r3"]
    with make("sb_n3_v1_e3_r3") as mc:
        res = mc.run()
        assert (res.status, res.violated, res.generated, res.distinct) == ("invariant", "NoSplitVote", g["generated"], 56)


def test_set_continue_after_init_is_refused():
    with make("n2_v1_e2_r3") as mc:
        mc.init()
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.set_continue()


def test_reset_zeroes_the_counts_and_keeps_the_setting():
    name = "n2_v1_e2_r3"
    with make(name) as mc:
        mc.set_continue()
        res = mc.run()
        check_run(name, mc, res)
        mc.reset()
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.violations()  # (before init)
        mc.init()
        # Init violates RaftCanCommt; nothing else is counted yet
        assert mc.violations() == {"RaftCanCommt": (1, 1), "FollowerCanCommit": (0, None), "CommitAll": (0, None)}
        res = mc.run()
        check_run(name, mc, res)
        check_traces(name, mc)


def test_resume_with_continuation_on_is_refused(tmp_path):
    path = str(tmp_path / "run.ckpt")
    with make("n2_v1_e2_r3") as a, make("n2_v1_e2_r3") as b:
        a.set_continue()
        a.init()
        a.step()
        a.checkpoint(path)  # (unaffected)
        b.set_continue()
        with pytest.raises(raftmc.RmcError, match="RMC_E_ARG.*violation counts"):
            b.resume(path)


def test_simulate_between_steps_leaves_the_counts():
    name = "n2_v1_e2_r3"
    e = CONT[name]
    with make(name, device_levels=1) as mc:
        mc.set_continue()
        mc.init()
        mc.step()
        before = mc.violations()
        sim = mc.simulate(64, depth=20, seed=1)
        # (the walks stop at their first error as without continuation: Init violates RaftCanCommt)
        assert sim.status == "invariant" and sim.violated == "RaftCanCommt"
        assert mc.violations() == before
        mc.step()
        assert mc.violation_levels("RaftCanCommt") == e["violations"]["RaftCanCommt"]["per_level"][:3]
        res = mc.run()
        check_run(name, mc, res)


# ---- 7. with coverage ---------------------------------------------------------------------------------------
def test_coverage_of_the_run_that_did_not_stop():
    name = "seeded_n3_v1_e2_r3"
    e = CONT[name]
    with make(name) as mc:
        mc.set_continue()
        mc.set_coverage()
        res = mc.run()
        check_run(name, mc, res)
        cov = mc.coverage()
    want = {"Init": (1, 1)}
    for a, act in enumerate(raftmc.ACTIONS):
        want[act] = (e["coverage"]["distinct"][a], e["coverage"]["generated"][a])
    assert cov == want


# ---- 8. launcher -------------------------------------------------------------------------------------------
COUNT_LINE = re.compile(r"^Invariant (\w+) is violated by (\d+) distinct states \(first at depth (\d+); the first "
                        r"behaviour is shown\)\.$")


def launch(tmp_path, args, module="Raft", **cfg):
    from test_gpu_coverage import spec_text
    from test_host import LAUNCHER, cfg_text
    (tmp_path / "Raft.cfg").write_text(cfg_text(**cfg))
    (tmp_path / f"{module}.tla").write_text(spec_text())
    env = dict(os.environ, RMC_SKIP_SPEC_CHECK="1")
    return subprocess.run([LAUNCHER] + args + ["-deadlock", "-config", str(tmp_path / "Raft.cfg"),
                           str(tmp_path / f"{module}.tla")], capture_output=True, text=True, env=env, timeout=120)


TIMED = re.compile(r"^(Starting|Finished|Progress|GPU:|Computing|Finished computing)")


@pytest.mark.parametrize("name,module,first,code,cfg", [
    ("sb_n3_v1_e3_r3", "RaftSplitBrain", "Error: The first argument of Assert evaluated to FALSE", 14,
     dict(E=3, R=3, vals="v1")),
    ("cpl_n3_v2_e1_r3", "RaftCommitPastLog", "Error: Evaluating invariant Inv failed.", 75, dict(E=1, R=3)),
])
def test_launcher_stopping_error_prints_as_without_continue(tmp_path, name, module, first, code, cfg):
    """The violation blocks come first; then the stopping error's own block, behaviour and closing counts,
    line for line what the run prints that checks Inv alone (never violated in either entry, so it stops at
    the same error with the same counters) without -continue."""
    e = CONT[name]
    r = launch(tmp_path, ["-continue"], module=module, inv="\n".join(e["invariants"]), **cfg)
    r0 = launch(tmp_path, [], module=module, inv="Inv", **cfg)
    assert r.returncode == r0.returncode == code, r.stdout + r.stderr
    out, out0 = r.stdout.splitlines(), r0.stdout.splitlines()

    def tail(lines):
        at = [i for i, ln in enumerate(lines) if ln.startswith(first)]
        assert len(at) == 1, lines
        return [ln for ln in lines[at[0]:] if not TIMED.match(ln)]

    assert tail(out) == tail(out0)
    states = [ln for ln in tail(out) if ln.startswith("State ")]
    assert len(states) > 1 and states[0] == "State 1: <Initial predicate>"
    if name == "cpl_n3_v2_e1_r3":  # the stop levels_errors.json records
        g = load("levels_errors.json")[name]
        assert len(states) == g["trace_len"]
        assert f"{g['generated']} states generated, {g['distinct']} distinct states found, {g['queue_left']} states " \
               "left on queue." in out
    assert any(ln.startswith(f"{e['generated']} states generated, {e['distinct']} distinct states found, ") for ln in out)
    counts = [(i, COUNT_LINE.match(ln)) for i, ln in enumerate(out) if COUNT_LINE.match(ln)]
    assert [(m.group(1), int(m.group(2)), int(m.group(3))) for _, m in counts] == \
        [(nm, v["count"], v["first_level"]) for nm, v in e["violations"].items() if v["count"]]
    assert counts[-1][0] < out.index(tail(out)[0])
    assert "Model checking completed. No error has been found." not in out


def test_launcher_prints_a_block_per_violated_invariant(tmp_path):
    name = "n2_v1_e2_r3"
    e = CONT[name]
    r = launch(tmp_path, ["-continue"], E=2, R=3, servers="s1, s2", vals="v1", inv="\n".join(e["invariants"]))
    assert r.returncode == 12, r.stdout + r.stderr
    out = r.stdout.splitlines()
    heads = [i for i, ln in enumerate(out) if ln.startswith("Error: Invariant ")]
    assert [out[i] for i in heads] == [f"Error: Invariant {nm} is violated." for nm in e["invariants"]]
    counts = [(i, COUNT_LINE.match(ln)) for i, ln in enumerate(out) if COUNT_LINE.match(ln)]
    assert [(m.group(1), int(m.group(2)), int(m.group(3))) for _, m in counts] == \
        [(nm, v["count"], v["first_level"]) for nm, v in e["violations"].items()]
    for k, nm in enumerate(e["invariants"]):
        block = out[heads[k]:counts[k][0]]
        assert block[1] == "Error: The behavior up to this point is:"
        states = [ln for ln in block if ln.startswith("State ")]
        assert len(states) == e["violations"][nm]["first_level"] and states[0] == "State 1: <Initial predicate>"
        assert k + 1 == len(heads) or counts[k][0] < heads[k + 1]
    assert "Model checking completed. No error has been found." not in out
    closing = f"{e['generated']} states generated, {e['distinct']} distinct states found, 0 states left on queue."
    assert closing in out and counts[-1][0] < out.index(closing)
    assert f"The depth of the complete state graph search is {e['depth']}." in out


def test_launcher_without_violations_prints_the_success_text(tmp_path):
    g = load("levels.json")["n3_v1_e1_r3"]
    r = launch(tmp_path, ["-continue"], E=1, R=3, vals="v1", inv="Inv")
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    assert "Model checking completed. No error has been found." in out
    assert f"{g['generated']} states generated, {g['distinct']} distinct states found, 0 states left on queue." in out
    assert not any(ln.startswith("Error:") or COUNT_LINE.match(ln) for ln in out)
    r0 = launch(tmp_path, [], E=1, R=3, vals="v1", inv="Inv")
    strip = [ln for ln in r0.stdout.splitlines() if not re.match(r"^(Starting|Finished|Progress|GPU:|Computing|Finished computing)", ln)]
    assert r0.returncode == 0 and strip == [ln for ln in out if not re.match(
        r"^(Starting|Finished|Progress|GPU:|Computing|Finished computing)", ln)]
