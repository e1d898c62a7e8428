"""Reachability queries (rmc_set_graph_keep / rmc_graph_reach; raftmc -canreach) without a device: the golden
fixture (tests/golden/reach.json, tests/golden/make_golden_reach.py) recomputed with numpy alone for the two
configurations whose whole graph is committed (graph_full.json.gz), its agreement with graph.json, the library's
exports and the launcher's refusals."""
import ctypes
import gzip
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import raftmc
import raft_ref as R
from conftest import GOLDEN, ROOT
from reach_ref import np_levels, np_query, np_shape, targets_of

LAUNCHER = os.path.join(ROOT, "tla-raft_amd", "build", "raftmc")
NAMES = ["n3_v1_e1_r3", "n2_v1_e2_r3", "nosym_n3_v1_e1_r3", "n3_v1_e2_r3", "seeded_n3_v1_e2_r3"]
FULL_KW = {"n3_v1_e1_r3": dict(n=3, V=1, max_election=1), "n2_v1_e2_r3": dict(n=2, V=1, max_election=2)}

with open(os.path.join(GOLDEN, "reach.json")) as _f:
    REACH = json.load(_f)
with open(os.path.join(GOLDEN, "graph.json")) as _f:
    GRAPH = json.load(_f)
with gzip.open(os.path.join(GOLDEN, "graph_full.json.gz")) as _f:
    FULL = json.load(_f)

QUERIES = [(b, name, v) for b, name in enumerate(raftmc.INVARIANT_BY_BIT) for v in (True, False)]


def qkey(name, value):
    return "%s=%s" % (name, "TRUE" if value else "FALSE")


def inv_values(cfg, states):
    out = np.zeros(len(states), dtype=np.uint16)
    for g, d in enumerate(states):
        st = R.state_from_json(d)
        for b, name in enumerate(raftmc.INVARIANT_BY_BIT):
            try:
                if R.INV_FUNCS[name](cfg, st):
                    out[g] |= 1 << b
            except R.EvalError:
                out[g] |= 1 << (8 + b)
    return out


def test_fixture_holds_the_five_configurations_and_fourteen_queries_each():
    assert list(REACH) == NAMES
    assert os.path.getsize(os.path.join(GOLDEN, "reach.json")) < (1 << 20)
    for name, e in REACH.items():
        assert (e["verdict"], e["states"], e["edges"]) == (GRAPH[name]["verdict"], GRAPH[name]["states"], GRAPH[name]["edges"])
        assert list(e["queries"]) == [qkey(n, v) for _b, n, v in QUERIES]
        assert e["level_starts"][0] == 0 and e["level_starts"] == sorted(set(e["level_starts"]))
        for q in e["queries"].values():
            assert q["can_reach"] + q["cannot_reach"] == e["states"] and q["targets"] <= q["can_reach"]
            assert [sum(x) for x in zip(*q["levels"])] == [q["can_reach"], q["cannot_reach"]]
            assert len(q["levels"]) == len(e["level_starts"])
            assert (q["first_cannot"] is None) == (q["cannot_reach"] == 0) == (q["first_cannot_level"] is None)
    assert (REACH["n3_v1_e2_r3"]["states"], REACH["n3_v1_e2_r3"]["edges"]) == (223437, 936729)
    assert REACH["seeded_n3_v1_e2_r3"]["verdict"] == "invariant"


def test_spot_values_of_the_specification():
    """RaftCanCommt = TRUE on the two smallest graphs, and their shape numbers."""
    want = {"n3_v1_e1_r3": (545, 300, 408, 137, 10, 9), "n2_v1_e2_r3": (1061, 706, 924, 137, 3, 6)}
    for name, w in want.items():
        e = REACH[name]
        q = e["queries"]["RaftCanCommt=TRUE"]
        assert (e["states"], q["targets"], q["can_reach"], q["cannot_reach"], q["first_cannot"], q["max_distance"]) == w
        assert e["cyclic_states"] == 0
    e = REACH["n2_v1_e2_r3"]
    assert (e["self_edges"], e["back_edges"], e["max_in"], e["max_out"], e["sinks"]) == (696, 7, 5, 5, 94)


@pytest.mark.parametrize("name", list(FULL_KW))
def test_numpy_fixpoint_reproduces_the_fixture(name):
    """Targets from the committed states through raft_ref.INV_FUNCS, distances by relaxing the edge arrays."""
    e = REACH[name]
    states = FULL[name]["states"]
    edges = np.array(FULL[name]["edges"], dtype=np.int64)
    src, dst = edges[:, 0], edges[:, 2]
    n = len(states)
    inv = inv_values(R.Config(max_restart=3, **FULL_KW[name]), states)
    assert hashlib.sha256(inv.astype("<u2").tobytes()).hexdigest() == e["inv_sha256"]
    sh = np_shape(n, src, dst)
    assert {k: sh[k] for k in ("states", "edges", "self_edges", "back_edges", "sinks", "max_in", "max_out", "cyclic_states")} == \
        {k: e[k] for k in ("states", "edges", "self_edges", "back_edges", "sinks", "max_in", "max_out", "cyclic_states")}
    lv = np_levels(n, src, dst)
    assert [int(np.flatnonzero(lv == k)[0]) for k in range(int(lv.max()) + 1)] == e["level_starts"]
    for b, inv_name, value in QUERIES:
        got, _dist = np_query(n, src, dst, targets_of(inv, b, value), lv)
        assert got == e["queries"][qkey(inv_name, value)], (inv_name, value)


def test_library_exports_the_reach_entry_points_within_abi_5():
    lib = raftmc.load_library()
    for f in ("rmc_set_graph_keep", "rmc_graph_reach", "rmc_graph_reach_levels", "rmc_graph_shape", "rmc_graph_inv_values",
              "rmc_graph_import"):
        assert hasattr(lib, f), f
    assert lib.rmc_abi_version() == 5
    assert ctypes.sizeof(raftmc._ReachQuery) == 8 and ctypes.sizeof(raftmc._ReachResult) == 88
    assert ctypes.sizeof(raftmc._GraphShape) == 8 * (8 + 128)
    header = open(os.path.join(ROOT, "include", "rmc.h")).read()
    assert "#define RMC_ABI_VERSION 5" in header
    for f in ("int rmc_set_graph_keep(void *ctx, int on);", "int rmc_graph_reach(", "int rmc_graph_reach_levels(",
              "int rmc_graph_shape(", "int rmc_graph_inv_values(", "int rmc_graph_import("):
        assert f in header, f
    for m in ("set_graph_keep", "graph_reach", "graph_reach_levels", "graph_shape", "graph_inv_values", "graph_import"):
        assert callable(getattr(raftmc.ModelChecker, m))


@pytest.mark.parametrize("args,word", [
    (["-canreach"], "-canreach"),
    (["-canreach", "RaftCanCommit", "Raft.tla"], "RaftCanCommit"),
    (["-canreach", "RaftCanCommt=MAYBE", "Raft.tla"], "RaftCanCommt=MAYBE"),
    (["-canreach", "RaftCanCommt", "-simulate", "Raft.tla"], "-simulate"),
    (["-canreach", "RaftCanCommt=FALSE", "-recover", "states", "Raft.tla"], "-recover"),
    (["-canreach", "RaftCanCommt", "-gpus", "2", "Raft.tla"], "-gpus"),
])
def test_launcher_canreach_usage_errors(args, word):
    """Refused before any file is read or a device touched."""
    r = subprocess.run([LAUNCHER] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 150, r.stdout + r.stderr
    first = r.stderr.splitlines()[0]
    assert word in first and "-canreach" in first and "unsupported option" not in first
    assert r.stdout == ""
    if len(args) > 1:
        assert "usage: raftmc" in r.stderr
