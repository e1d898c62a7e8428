"""The high-term fixtures (tests/golden/make_golden_highterm.py: MaxElection 4..7, MaxRestart up to 7)
against the oracle in the tree, and the message-universe limit where no device is needed.

The fixtures exist to put currentTerm / electionCount / log-entry terms of 4..7, restartCount above 3 and
message terms of 4..7 through the kernels (tests/test_gpu_highterm.py).  Here: the states they hold do have
those values (the coverage conditions, recomputed from the states, not read from the recorded counts), the
recorded successors, classes and invariant values are what oracle/raft_ref.py computes now, and a
configuration whose message universe does not fit the 16-bit ids is refused by the cfg parser, by rmc_create
(before it looks for a device) and by the launcher, each naming the pair's largest MaxElection."""
import gzip
import json
import os
import random
import subprocess
import sys

import pytest

import raft_ref as R
import raftmc
from conftest import GOLDEN
from test_host import LAUNCHER, cfg_text

sys.path.insert(0, GOLDEN)
import make_golden_highterm as G  # noqa: E402  (COVER, properties, coverage_counts: the generator's definitions)

with gzip.open(os.path.join(GOLDEN, "successors_highterm.json.gz"), "rt") as _f:
    HIGH = json.load(_f)
with open(os.path.join(GOLDEN, "levels_highterm.json")) as _f:
    LEVELS = json.load(_f)
INV_NAMES = ["Inv", "NoSplitVote", "RaftCanCommt", "FollowerCanCommit", "CommitAll", "NoAllCommit",
             "ExistLeaderAndCandidate"]


def test_fixture_holds_the_named_configurations():
    assert sorted(HIGH) == sorted(name for name, *_ in G.CONFIGS)
    for name, n, V, E, Rr, bf, keep, mcap in G.CONFIGS:
        g = HIGH[name]
        assert (g["n"], g["V"], g["E"], g["R"], g["become_follower"], g["msg_cap"]) == (n, V, E, Rr, bf, mcap)
        assert len(g["items"]) == keep and not any(it["synthetic"] for it in g["items"])
    want = [f"n{n}_v{V}_e{E}_r{Rr}" for n, V, E, Rr in G.BOTH + G.C_ONLY + G.E0]
    want += [f"deadlock_n{n}_v{V}_e{E}_r{Rr}" for n, V, E, Rr in G.E0]
    want += [f"n{n}_v{V}_e{E}_r{Rr}" for n, V, E, Rr, _ in G.PREFIXES]
    assert sorted(LEVELS) == sorted(want)


@pytest.mark.parametrize("name", sorted(HIGH))
def test_coverage_conditions_hold(name):
    """Recomputed from the kept states: every configuration with E >= 6 has at least 10 states with a
    currentTerm = E, 10 with electionCount = E, 10 with a log entry of term >= 4, 5 with restartCount >= 4,
    10 holding a message of term >= 4, one an AppendReq with prevLogTerm >= 4, one a VoteReq with
    lastLogTerm >= 4 -- and the recorded counts are those."""
    g = HIGH[name]
    states = [it["state"] for it in g["items"]]
    cov = G.coverage_counts(states, g["E"])
    for k, v in cov.items():
        assert g["coverage"][k] == v, k
    assert g["E"] >= 6
    assert dict(G.COVER) == dict(append_req_prev_log_term_ge4=1, vote_req_last_log_term_ge4=1, restart_count_ge4=5,
                                 current_term_top=10, election_count_top=10, log_term_ge4=10, msg_term_ge4=10)
    for prop, least in G.COVER:
        assert cov[prop] >= least, (prop, cov[prop])
    # the properties as the issue words them, not through the generator's function
    E = g["E"]
    assert sum(1 for d in states if E in d["currentTerm"]) >= 10
    assert sum(1 for d in states if d["electionCount"] == E) >= 10
    assert sum(1 for d in states if any(t >= 4 for log in d["logs"] for t, _ in log)) >= 10
    assert sum(1 for d in states if d["restartCount"] >= 4) >= 5
    assert sum(1 for d in states if any(m["term"] >= 4 for m in d["msgs"])) >= 10
    assert any(m["type"] == "AppendReq" and m["prevLogTerm"] >= 4 for d in states for m in d["msgs"])
    assert any(m["type"] == "VoteReq" and m["lastLogTerm"] >= 4 for d in states for m in d["msgs"])
    assert cov["max_current_term"] == E and cov["max_election_count"] == E and cov["max_msg_term"] == E
    if g["become_follower"]:
        assert g["coverage"]["become_follower_successors"] > 0


@pytest.mark.parametrize("name", sorted(HIGH))
def test_fixture_reproduced_by_the_python_oracle(name):
    """10 states per configuration (seeded): raft_ref.successors / canonical / the invariants give the
    recorded successor lists, the recorded partition into classes and the recorded invariant values."""
    g = HIGH[name]
    cfg = R.Config(n=g["n"], V=g["V"], max_election=g["E"], max_restart=g["R"], become_follower=g["become_follower"])
    rng = random.Random(20261021)
    items = rng.sample(g["items"], 10)
    id_of_canon, canon_of_id = {}, {}
    for it in items:
        st = R.state_from_json(it["state"])
        assert R.state_to_json(st) == it["state"] and it["nmsgs"] == len(st.msgs) and not it["assert_fails"]
        succ = R.successors(cfg, st)
        assert [list(k) for k, _ in succ] == [e["key"] for e in it["successors"]]
        assert [R.state_to_json(t) for _, t in succ] == [e["state"] for e in it["successors"]]
        assert R.canonical(cfg, R.state_from_json(it["permuted"])) == R.canonical(cfg, st)
        for (_, t), e in zip(succ, it["successors"]):
            c = R.canonical(cfg, t)
            assert id_of_canon.setdefault(c, e["canon"]) == e["canon"]
            assert canon_of_id.setdefault(e["canon"], c) == c
        for tag, vals in it["invariants"].items():
            t = st if tag == "state" else succ[int(tag[4:])][1]
            got = []
            for nm in INV_NAMES:
                try:
                    got.append(R.INV_FUNCS[nm](cfg, t))
                except R.EvalError:
                    got.append(None)
            assert got == vals, tag


def test_levels_fixture_shape():
    """The exhausted entries are whole runs (levels.json's format), the prefixes complete levels only
    (levels_prefix.json's); the prefixes reach a level that holds states of term 7 (level 8 at the latest:
    seven elections from Init), and the E = 0 entries are Init alone."""
    for name, g in LEVELS.items():
        assert g["invariants"] == ["Inv"], name
        assert max(g["E"], g["R"]) >= 4 or min(g["E"], g["R"]) == 0, name
        if g["exhausted"]:
            assert g["distinct"] == sum(g["levels"]) and g["depth"] == len(g["levels"]) == len(g["gen_per_level"])
            assert g["generated"] == 1 + sum(g["gen_per_level"])
        else:
            assert len(g["gen_per_level"]) == len(g["levels"]) - 1 and len(g["levels"]) >= 8
            assert sum(g["levels"]) <= g["stopped_at_distinct"]
    for name in ("n2_v1_e0_r3", "n3_v1_e0_r15"):
        g, gd = LEVELS[name], LEVELS["deadlock_" + name]
        assert (g["verdict"], g["distinct"], g["generated"], g["depth"], g["levels"]) == ("ok", 1, 1, 1, [1])
        assert (gd["verdict"], gd["distinct"], gd["generated"], gd["trace_len"], gd["queue_left"]) == ("deadlock", 1, 1, 1, 0)
    assert LEVELS["n2_v1_e4_r3"]["distinct"] == 219772 and LEVELS["n2_v1_e4_r3"]["depth"] == 40
    assert LEVELS["n3_v1_e1_r0"]["distinct"] == 276 and LEVELS["n2_v1_e2_r0"]["distinct"] == 327
    assert LEVELS["n3_v2_e1_r0"]["distinct"] == 5254


def test_small_levels_reproduced_by_the_python_oracle():
    for name in ("n2_v1_e2_r0", "n3_v1_e1_r0", "n2_v1_e0_r3", "deadlock_n3_v1_e0_r15"):
        g = LEVELS[name]
        p = R.bfs(R.Config(n=g["n"], V=g["V"], max_election=g["E"], max_restart=g["R"],
                           check_deadlock=g["check_deadlock"]))
        assert (p.verdict, p.generated, p.distinct, p.levels, p.generated_per_level) == \
               (g["verdict"], g["generated"], g["distinct"], g["levels"], g["gen_per_level"]), name


# ---- the message-universe limit (16-bit message ids; rmc_spec.h max_election_limit) ---------------------
# (servers, values) -> the largest MaxElection whose universe has fewer than 0xFFFF records
LIMITS = {(2, 1): 7, (2, 2): 7, (3, 1): 7, (4, 1): 7, (5, 1): 7, (3, 2): 6, (3, 3): 4, (4, 2): 5, (5, 2): 4}


def universe_records(n, V, E):
    """rmc_spec.h make_dims(n, V, E).total: VoteReq + VoteResp + AppendReq + AppendResp records."""
    P, v1 = n * n, V + 1
    return P * E * v1 * (E + 1) + P * E + P * E * v1 * (E + 1) * (1 + E * V) * v1 + P * E * v1 * 2


def test_limits_follow_from_the_universe_size():
    for (n, V), lim in LIMITS.items():
        assert universe_records(n, V, lim) < 0xFFFF
        assert lim == 7 or universe_records(n, V, lim + 1) >= 0xFFFF
    assert [universe_records(*x) for x in ((3, 2, 7), (3, 3, 5), (4, 2, 6), (5, 2, 5))] == [69993, 70605, 81312, 77375]


def _cfg(n, V, E):
    return cfg_text(E=E, R=3, servers=", ".join(f"s{i + 1}" for i in range(n)),
                    vals=", ".join(f"v{i + 1}" for i in range(V)))


@pytest.mark.parametrize("n,V", sorted(LIMITS))
def test_parse_config_reports_the_limit(n, V):
    lim = LIMITS[(n, V)]
    c = raftmc.parse_config(_cfg(n, V, lim))
    assert (c.n_servers, c.n_vals, c.max_election) == (n, V, lim)
    if lim < 7:
        with pytest.raises(raftmc.RmcError, match=rf"MaxElection = {lim + 1} .*MaxElection is at most {lim} for this pair"):
            raftmc.parse_config(_cfg(n, V, lim + 1))
        with pytest.raises(raftmc.RmcError, match=rf"MaxElection is at most {lim} for this pair"):
            raftmc.parse_config(_cfg(n, V, 7))


@pytest.mark.parametrize("n,V,E", [(3, 2, 7), (3, 3, 5), (4, 2, 6), (5, 2, 5)])
def test_create_refuses_an_oversized_universe_before_the_device(n, V, E):
    """RMC_E_ARG with the pair's limit in the text, on a machine with or without a GPU: the check is host
    arithmetic ahead of device selection (a machine without one would answer RMC_E_DEVICE otherwise)."""
    with pytest.raises(raftmc.RmcError, match=rf"RMC_E_ARG: .*max_election is at most {LIMITS[(n, V)]} for this pair"):
        raftmc.ModelChecker(raftmc.ModelConfig(n_servers=n, n_vals=V, max_election=E, max_restart=3))


def test_launcher_rejects_an_oversized_universe(tmp_path):
    """raftmc prints the parser's message and leaves with the cfg-error code, before it opens a device."""
    (tmp_path / "Raft.cfg").write_text(_cfg(3, 2, 7))
    env = dict(os.environ, RMC_SKIP_SPEC_CHECK="1")
    r = subprocess.run([LAUNCHER, "-deadlock", "-config", str(tmp_path / "Raft.cfg"), str(tmp_path / "Raft.tla")],
                       capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 151, r.stdout + r.stderr
    assert "Error: CONSTANT MaxElection = 7 is too large for 3 servers and 2 values" in r.stdout
    assert "MaxElection is at most 6 for this pair" in r.stdout
    assert "could not start the GPU model checker" not in r.stdout
