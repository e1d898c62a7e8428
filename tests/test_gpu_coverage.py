"""Action coverage on the GPU (rmc_set_coverage / rmc_get_coverage; raftmc -coverage): per action, the
successors generated and the states first found, against tests/golden/coverage.json (the Python oracle,
tests/golden/make_golden_coverage.py).  Integers: every comparison is exact.

Every execution path counts: fused small levels (the device loop steps aside while coverage is on),
host-driven chunks, split chunks with look-ahead, virtual shards with and without replicated levels, the
one-rank RCCL communicator and two rank processes over the host transport.  The four error
configurations (invariant, Assert, deadlock, evaluation error) are the ones a wrong cut at the error
would fail."""
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


COVERAGE = load("coverage.json")
LEVELS_OF = {f: load(f) for f in sorted({e["levels_file"] for e in COVERAGE.values()})}
ERRORS = ["seeded_n3_v1_e2_r3", "sb_n3_v1_e2_r3", "deadlock_n3_v1_e1_r3", "cpl_n3_v2_e1_r3"]


def golden(name):
    return LEVELS_OF[COVERAGE[name]["levels_file"]][name]


def cfg_kw(name, **kw):
    g = golden(name)
    if name.startswith("nosym_"):
        kw["symmetry"] = False
    return dict(n_servers=g["n"], n_vals=g["V"], max_election=g["E"], max_restart=g["R"],
                invariants=tuple(g["invariants"]), check_deadlock=g["check_deadlock"], spec_variant=spec_of(g), **kw)


def make(name, **kw):
    return raftmc.ModelChecker(raftmc.ModelConfig(**cfg_kw(name, **kw)))


def as_cov(gen, dist):
    out = {"Init": (1, 1)}
    for a, act in enumerate(raftmc.ACTIONS):
        out[act] = (dist[a], gen[a])
    return out


def expected(name):
    return as_cov(COVERAGE[name]["generated"], COVERAGE[name]["distinct"])


def run_covered(name, **kw):
    with make(name, **kw) as mc:
        mc.set_coverage()
        res = mc.run()
        check_levels(golden(name), res)
        cov = mc.coverage()
    assert 1 + sum(v[1] for k, v in cov.items() if k != "Init") == res.generated
    assert 1 + sum(v[0] for k, v in cov.items() if k != "Init") == res.distinct
    return cov


# ---- 1. fused small levels, default settings -------------------------------------------------------------
def test_fixture_covers_the_kernel_variants():
    assert len(COVERAGE) == 12 and all(n in COVERAGE for n in ERRORS)
    g = {n: golden(n) for n in COVERAGE}
    assert {g[n]["n"] for n in COVERAGE} == {2, 3, 4, 5} and {g[n]["V"] for n in COVERAGE} == {1, 2}
    assert golden("bf_n3_v1_e1_r3").get("become_follower")


@pytest.mark.parametrize("name", list(COVERAGE))
def test_coverage_matches_golden_default_settings(name):
    assert run_covered(name) == expected(name)


# ---- 2. level boundaries ----------------------------------------------------------------------------------
def test_coverage_after_every_level_matches_golden():
    pl = COVERAGE["n3_v1_e1_r3"]["per_level"]
    with make("n3_v1_e1_r3", device_levels=1) as mc:
        mc.set_coverage()
        mc.init()
        assert mc.coverage() == as_cov([0] * 13, [0] * 13)
        for k, p in enumerate(pl):
            ls = mc.step()
            assert mc.coverage() == as_cov(p["generated"], p["distinct"]), k
        assert ls.status == "done"


@pytest.mark.parametrize("device_levels", [0, 4])
def test_coverage_does_not_depend_on_device_levels(device_levels):
    assert run_covered("n3_v1_e1_r3", device_levels=device_levels) == expected("n3_v1_e1_r3")


# ---- 3. split chunks with look-ahead ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n3_v1_e2_r3", "n4_v1_e1_r3", "bf_n3_v1_e1_r3", "seeded_n3_v1_e2_r3",
                                  "cpl_n3_v2_e1_r3"])
def test_coverage_split_chunks_with_lookahead(name, monkeypatch):
    monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    assert run_covered(name, device_levels=1, chunk_successors=6000) == expected(name)


# ---- 4. sharded --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [2, 3])
@pytest.mark.parametrize("name", ["n3_v1_e2_r3", "seeded_n3_v1_e2_r3", "sb_n3_v1_e2_r3"])
def test_coverage_virtual_shards(name, shards):
    assert run_covered(name, virtual_shards=shards, chunk_successors=3000, shard_min_states=1) == expected(name)


def test_coverage_counts_replicated_levels_once():
    assert run_covered("n3_v1_e1_r3", virtual_shards=2, chunk_successors=3000, shard_min_states=40) == \
        expected("n3_v1_e1_r3")


def test_coverage_one_rank_rccl():
    assert run_covered("n3_v1_e2_r3", world_size=1, rank=0, comm_unique_id=raftmc.comm_unique_id(),
                       chunk_successors=3000, shard_min_states=1) == expected("n3_v1_e2_r3")


def test_coverage_two_rank_processes_over_the_host_transport(tmp_path):
    """Each rank counts its own parents and winners; the rounds' all-reduces sum them, so both report the
    global totals."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    name = "n3_v1_e1_r3"
    cfg = cfg_kw(name, chunk_successors=3000, shard_min_states=1)
    cfg["invariants"] = list(cfg["invariants"])
    procs, outs = [], []
    for r in range(2):
        outs.append(str(tmp_path / f"rank{r}.json"))
        spec = dict(rank=r, world=2, port=port, cfg=cfg, out=outs[-1])
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "coverage_worker.py"), json.dumps(spec)],
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
    g = golden(name)
    for o in outs:
        with open(o) as f:
            r = json.load(f)
        assert "error" not in r, r.get("error")
        assert (r["status"], r["generated"], r["distinct"]) == ("done", g["generated"], g["distinct"])
        assert {k: tuple(v) for k, v in r["coverage"].items()} == expected(name)


# ---- 5. lifecycle ------------------------------------------------------------------------------------------
def test_coverage_is_off_by_default():
    with make("n3_v1_e1_r3") as mc:
        res = mc.run()
        check_levels(golden("n3_v1_e1_r3"), res)
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.coverage()


def test_set_coverage_after_init_is_refused():
    with make("n3_v1_e1_r3") as mc:
        mc.init()
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.set_coverage()


def test_reset_zeroes_the_counts_and_keeps_the_setting():
    name = "seeded_n3_v1_e2_r3"
    with make(name) as mc:
        mc.set_coverage()
        mc.run()
        first = mc.coverage()
        mc.reset()
        mc.init()
        assert mc.coverage() == as_cov([0] * 13, [0] * 13)
        mc.run()
        assert mc.coverage() == first == expected(name)


def test_resume_with_coverage_on_is_refused(tmp_path):
    path = str(tmp_path / "run.ckpt")
    with make("n3_v1_e1_r3") as a, make("n3_v1_e1_r3") as b:
        a.init()
        a.step()
        a.checkpoint(path)
        b.set_coverage()
        with pytest.raises(raftmc.RmcError, match="RMC_E_ARG.*coverage"):
            b.resume(path)


def test_simulate_between_steps_leaves_the_counts():
    pl = COVERAGE["n3_v1_e1_r3"]["per_level"]
    with make("n3_v1_e1_r3", device_levels=1) as mc:
        mc.set_coverage()
        mc.init()
        mc.step()
        sim = mc.simulate(64, depth=20, seed=1)
        assert sim.walks == 64 and sim.generated > 0
        assert mc.coverage() == as_cov(pl[0]["generated"], pl[0]["distinct"])
        mc.step()
        assert mc.coverage() == as_cov(pl[1]["generated"], pl[1]["distinct"])


# ---- 6. launcher -------------------------------------------------------------------------------------------
NEXT_ORDER = ["BecomeCandidate", "UpdateTerm", "ResponseVote", "BecomeLeader", "ClientReq", "LeaderAppendEntry",
              "FollowerAcceptEntry", "FollowerRejectEntry", "HandleAppendResp", "LeaderCanCommit", "Restart"]
LINE = re.compile(r"^<(\w+) line .* of module \w+>: (\d+):(\d+)$")


def spec_text():
    """A module text with a definition per name the report locates (the launcher reads it for the source
    ranges only: RMC_SKIP_SPEC_CHECK=1)."""
    out = ["---- MODULE Raft ----", "Init ==", "    /\\ TRUE", ""]
    for act in NEXT_ORDER:
        out += [f"{act}(s) ==", "    /\\ TRUE", "    /\\ UNCHANGED <<s>>", ""]
    return "\n".join(out + ["===="]) + "\n"


def test_launcher_prints_the_coverage_block(tmp_path):
    from test_host import LAUNCHER, cfg_text
    name = "n3_v1_e1_r3"
    g, e = golden(name), COVERAGE[name]
    (tmp_path / "Raft.cfg").write_text(cfg_text(E=g["E"], R=g["R"], vals="v1"))
    (tmp_path / "Raft.tla").write_text(spec_text())
    env = dict(os.environ, RMC_SKIP_SPEC_CHECK="1")
    base = [LAUNCHER, "-deadlock", "-config", str(tmp_path / "Raft.cfg"), str(tmp_path / "Raft.tla")]
    r = subprocess.run(base[:1] + ["-coverage", "1"] + base[1:], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.splitlines()
    got = [(m.group(1), int(m.group(2)), int(m.group(3))) for m in map(LINE.match, out) if m]
    assert got == [("Init", 1, 1)] + [(a, e["distinct"][raftmc.ACTIONS.index(a)], e["generated"][raftmc.ACTIONS.index(a)])
                                      for a in NEXT_ORDER]
    closing = f"{g['generated']} states generated, {g['distinct']} distinct states found, 0 states left on queue."
    start = [i for i, ln in enumerate(out) if ln.startswith("The coverage statistics at ")]
    assert len(start) == 1 and "End of statistics." in out
    assert out.index("Model checking completed. No error has been found.") < start[0] < out.index("End of statistics.") \
        < out.index(closing)
    r0 = subprocess.run(base, capture_output=True, text=True, env=env, timeout=120)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    out0 = r0.stdout.splitlines()
    assert closing in out0 and not any(LINE.match(ln) for ln in out0)
    assert "End of statistics." not in out0 and not any("coverage statistics" in ln for ln in out0)
