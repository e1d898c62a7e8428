"""Liveness over the kept state graph (rmc_graph_eventually / rmc_graph_avoid_path / rmc_graph_scc; raftmc -eventually,
-leadsto, -scc) without a device: the golden fixture (tests/golden/live.json, tests/golden/make_golden_live.py)
recomputed with tests/live_ref.py for the two configurations whose whole graph is committed (graph_full.json.gz), its
agreement with reach.json, the library's exports and the launcher's refusals."""
import ctypes
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import raftmc
import raft_ref as R
from conftest import GOLDEN, ROOT
from live_ref import UNSET, np_live_query, np_scc, scc_summary
from reach_ref import np_dist, np_levels, targets_of
from test_reach_host import FULL_KW, NAMES, inv_values

LAUNCHER = os.path.join(ROOT, "tla-raft_amd", "build", "raftmc")

with open(os.path.join(GOLDEN, "live.json")) as _f:
    LIVE = json.load(_f)
with open(os.path.join(GOLDEN, "reach.json")) as _f:
    REACH = json.load(_f)
with gzip.open(os.path.join(GOLDEN, "graph_full.json.gz")) as _f:
    FULL = json.load(_f)

TRUE_KEYS = ["%s=TRUE" % n for n in raftmc.INVARIANT_BY_BIT]
KEYS = TRUE_KEYS + ["RaftCanCommt=FALSE", "CommitAll=FALSE", "ExistLeaderAndCandidate=TRUE~>RaftCanCommt=TRUE",
                    "RaftCanCommt=TRUE~>CommitAll=TRUE"]


def sets_of(inv, key):
    """(target, source or None) as bool arrays for a live.json query key"""
    def one(s):
        name, value = s.split("=")
        return targets_of(inv, raftmc.INVARIANT_BY_BIT.index(name), value == "TRUE")
    src, _, tgt = key.rpartition("~>")
    return one(tgt), one(src) if src else None


def test_fixture_holds_the_five_configurations_and_their_queries():
    assert list(LIVE) == NAMES
    assert os.path.getsize(os.path.join(GOLDEN, "live.json")) < (1 << 20)
    for name, e in LIVE.items():
        r = REACH[name]
        assert (e["verdict"], e["states"], e["edges"], e["level_starts"], e["inv_sha256"]) == \
            (r["verdict"], r["states"], r["edges"], r["level_starts"], r["inv_sha256"])
        assert list(e["queries"]) == KEYS
        for key, q in e["queries"].items():
            assert q["must"] + q["avoiders"] == e["states"] and q["targets"] <= q["must"]
            assert [sum(x) for x in zip(*q["levels"])] == [q["must"], q["avoiders"]]
            assert len(q["levels"]) == len(e["level_starts"])
            assert (q["first_avoid"] is None) == (q["avoiders"] == 0) == (q["avoid_path"] is None)
            assert q["avoid_terminal"] <= q["avoiders"]
            # what must reach P can reach it; a state that cannot reach P is an avoider
            tgt = key.rpartition("~>")[2]
            assert q["targets"] == r["queries"][tgt]["targets"]
            assert q["must"] <= r["queries"][tgt]["can_reach"] and q["max_within"] >= 0
            if q["avoid_path"] is not None:
                assert q["avoid_path"]["gids"][0] == q["first_avoid"]
            if "~>" in key:
                assert q["source_avoiders"] <= min(q["sources"], q["avoiders"])
                assert (q["source_avoiders"] == 0) == (q["first_source_avoid"] is None) == (q["source_path"] is None)
        # nontrivial components exactly where the peeling leaves states: every Raft graph measured is acyclic
        assert (e["scc"]["nontrivial"] == 0) == (r["cyclic_states"] == 0)
        assert e["scc"]["nontrivial_states"] <= r["cyclic_states"]
        if e["scc"]["nontrivial"] == 0:
            assert e["scc"] == dict(components=e["states"], nontrivial=0, nontrivial_states=0, largest=1)
            for q in e["queries"].values():  # no cycle: every counterexample ends in a state with no step out
                assert q["avoid_path"] is None or q["avoid_path"]["loop_at"] is None
    assert LIVE["seeded_n3_v1_e2_r3"]["verdict"] == "invariant"
    assert LIVE["n3_v1_e2_r3"]["states"] == 223437


@pytest.mark.parametrize("name", list(FULL_KW))
def test_references_reproduce_the_fixture(name):
    """Targets from the committed states through raft_ref.INV_FUNCS; within, the walks and the components from
    tests/live_ref.py; must inside can_reach and within >= dist against reach_ref's distances."""
    e = LIVE[name]
    states = FULL[name]["states"]
    edges = np.array(FULL[name]["edges"], dtype=np.int64)
    src, dst = edges[:, 0], edges[:, 2]
    n = len(states)
    inv = inv_values(R.Config(max_restart=3, **FULL_KW[name]), states)
    lv = np_levels(n, src, dst)
    for key in KEYS:
        target, source = sets_of(inv, key)
        got, within = np_live_query(n, src, dst, target, lv, source)
        assert got == e["queries"][key], key
        dist = np_dist(n, src, dst, target)
        m = within != UNSET
        assert (dist[m] != UNSET).all() and (within[m] >= dist[m]).all()
        assert ((within == 0) == target).all()
    label = np_scc(n, src, dst)
    assert scc_summary(label) == e["scc"] and np.array_equal(label, np.arange(n))


def test_references_on_small_graphs():
    """The references against values worked out by hand (they are what the GPU tests compare with)."""
    # diamond with branches of length 1 and 3 into the target 5
    q, w = np_live_query(6, [0, 1, 0, 2, 3, 4], [1, 5, 2, 3, 4, 5], np.array([0, 0, 0, 0, 0, 1], dtype=bool))
    assert w.tolist() == [4, 1, 3, 2, 1, 0] and q["avoiders"] == 0
    # 0 -> 1 <-> 2 -> 3 (target): a lasso from 0 that closes at index 1
    q, w = np_live_query(4, [0, 1, 2, 2], [1, 2, 1, 3], np.array([0, 0, 0, 1], dtype=bool))
    assert w.tolist() == [UNSET, UNSET, UNSET, 0] and q["avoid_path"] == dict(gids=[0, 1, 2], loop_at=1)
    assert q["avoid_terminal"] == 0
    # a sink that is no target below 0, which also has an edge to the target 1
    q, w = np_live_query(3, [0, 0], [1, 2], np.array([0, 1, 0], dtype=bool))
    assert w.tolist() == [UNSET, 0, UNSET] and q["avoid_path"] == dict(gids=[0, 2], loop_at=None)
    assert np_scc(6, [0, 1, 2, 2, 3, 4, 5], [1, 2, 0, 3, 4, 5, 3]).tolist() == [0, 0, 0, 3, 3, 3]
    assert np_scc(7, [4, 3, 2, 1, 6, 5], [3, 2, 1, 4, 5, 4]).tolist() == [0, 1, 1, 1, 1, 5, 6]
    assert np_scc(3, [0, 1, 2], [0, 1, 2]).tolist() == [0, 1, 2]


def test_library_exports_the_live_entry_points_within_abi_5():
    lib = raftmc.load_library()
    for f in ("rmc_graph_eventually", "rmc_graph_eventually_levels", "rmc_graph_avoid_path", "rmc_graph_scc"):
        assert hasattr(lib, f), f
    assert lib.rmc_abi_version() == 5
    assert ctypes.sizeof(raftmc._LiveQuery) == 16 and ctypes.sizeof(raftmc._LiveResult) == 128
    assert ctypes.sizeof(raftmc._SccResult) == 64
    header = open(os.path.join(ROOT, "include", "rmc.h")).read()
    assert "#define RMC_ABI_VERSION 5" in header
    for f in ("int rmc_graph_eventually(void *ctx, const rmc_live_query *q, rmc_live_result *res, uint32_t *within_out);",
              "int rmc_graph_eventually_levels(", "int rmc_graph_avoid_path(", "int rmc_graph_scc("):
        assert f in header, f
    for m in ("graph_eventually", "graph_eventually_levels", "graph_avoid_path", "graph_scc"):
        assert callable(getattr(raftmc.ModelChecker, m))


@pytest.mark.parametrize("args,words", [
    (["-eventually"], ["-eventually"]),
    (["-eventually", "RaftCanCommit", "Raft.tla"], ["-eventually", "RaftCanCommit"]),
    (["-eventually", "RaftCanCommt=MAYBE", "Raft.tla"], ["-eventually", "RaftCanCommt=MAYBE"]),
    (["-eventually", "RaftCanCommt", "-simulate", "Raft.tla"], ["-eventually", "-simulate"]),
    (["-eventually", "RaftCanCommt=FALSE", "-recover", "states", "Raft.tla"], ["-eventually", "-recover"]),
    (["-eventually", "RaftCanCommt", "-gpus", "2", "Raft.tla"], ["-eventually", "-gpus"]),
    (["-leadsto", "RaftCanCommt", "Raft.tla"], ["-leadsto", "two arguments"]),
    (["-leadsto", "RaftCanCommt"], ["-leadsto", "two arguments"]),
    (["-leadsto", "RaftCanCommt", "CommitAl", "Raft.tla"], ["-leadsto", "CommitAl"]),
    (["-leadsto", "NoSuch=FALSE", "CommitAll", "Raft.tla"], ["-leadsto", "NoSuch=FALSE"]),
    (["-leadsto", "RaftCanCommt", "CommitAll", "-simulate", "Raft.tla"], ["-leadsto", "-simulate"]),
    (["-leadsto", "RaftCanCommt", "CommitAll=FALSE", "-gpus", "2", "Raft.tla"], ["-leadsto", "-gpus"]),
    (["-scc", "-simulate", "Raft.tla"], ["-scc", "-simulate"]),
    (["-scc", "-recover", "states", "Raft.tla"], ["-scc", "-recover"]),
    (["-scc", "-gpus", "2", "Raft.tla"], ["-scc", "-gpus"]),
])
def test_launcher_usage_errors(args, words):
    """Refused before any file is read or a device touched."""
    r = subprocess.run([LAUNCHER] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 150, r.stdout + r.stderr
    first = r.stderr.splitlines()[0]
    assert all(w in first for w in words) and "unsupported option" not in first
    assert r.stdout == ""
    if len(args) > 1:
        assert "usage: raftmc" in r.stderr


@pytest.mark.parametrize("flags", [["-eventually", "RaftCanCommt"], ["-eventually", "CommitAll=FALSE"],
                                   ["-leadsto", "RaftCanCommt", "CommitAll"], ["-leadsto", "Inv=FALSE", "NoAllCommit=TRUE"],
                                   ["-scc"], ["-eventually", "Inv", "-leadsto", "Inv", "CommitAll", "-scc", "-canreach", "Inv"]])
def test_launcher_accepts_the_flags(flags, tmp_path):
    """Accepted: the run goes on to read the cfg (there is none: exit 151), never "unsupported option"."""
    r = subprocess.run([LAUNCHER] + flags + ["-config", str(tmp_path / "none.cfg"), str(tmp_path / "Raft.tla")],
                       capture_output=True, text=True, timeout=60, env=dict(os.environ, RMC_SKIP_SPEC_CHECK="1"))
    assert r.returncode == 151, r.stdout + r.stderr
    assert "unsupported option" not in r.stderr and "usage: raftmc" not in r.stderr
    assert "cannot read" in r.stderr
