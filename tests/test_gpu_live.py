"""Liveness over the kept state graph on the GPU (rmc_graph_eventually / rmc_graph_avoid_path / rmc_graph_scc; raftmc
-eventually, -leadsto, -scc): the kept graph of a run against tests/golden/live.json (the Python oracle,
tests/golden/make_golden_live.py), and the kernels on imported graphs against the references of tests/live_ref.py.
Integers and digests: every comparison is exact.  Every test fails without the feature (the entry points do not
exist)."""
import gzip
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import raftmc
from conftest import GOLDEN
from live_ref import UNSET, live_fields, np_live_query, np_scc, np_within, scc_summary
from reach_ref import np_levels, targets_of
from test_gpu_coverage import cfg_kw
from test_reach_host import FULL_KW, inv_values
from tla_render import render_state

import raft_ref as R

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "live.json")) as _f:
    LIVE = json.load(_f)
with gzip.open(os.path.join(GOLDEN, "graph_full.json.gz")) as _f:
    FULL = json.load(_f)
RUNS = ["n3_v1_e1_r3", "n3_v1_e2_r3", "seeded_n3_v1_e2_r3"]
SCC_KEYS = ("components", "nontrivial", "nontrivial_states", "largest")


def make(name, **kw):
    return raftmc.ModelChecker(raftmc.ModelConfig(**cfg_kw(name, **kw)))


def parse_key(key):
    """live.json's query key -> graph_eventually's arguments"""
    src, _, tgt = key.rpartition("~>")
    name, value = tgt.split("=")
    kw = dict(invariant=name, value=value == "TRUE")
    if src:
        sname, svalue = src.split("=")
        kw.update(source=sname, source_value=svalue == "TRUE")
    return kw


def scc_fields(r):
    return {k: getattr(r, k) for k in SCC_KEYS}


# ---- a. runs against the fixture ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", RUNS)
def test_run_equals_the_fixture(name):
    e = LIVE[name]
    with make(name) as mc:
        mc.set_graph_keep()
        res = mc.run()
        assert res.status == ("done" if e["verdict"] == "ok" else e["verdict"]) and res.distinct == e["states"]
        for key, want in e["queries"].items():
            r = mc.graph_eventually(want_within=True, **parse_key(key))
            got = live_fields(mc, r, mc.graph_eventually_levels())
            got["within_sha256"] = hashlib.sha256(r.within.astype("<u4").tobytes()).hexdigest()
            assert got == want, key
            assert (r.states, r.edges) == (e["states"], e["edges"])
            assert r.within.dtype == np.uint32 and r.rounds == (r.max_within + 1 if r.targets else 0)
        s = mc.graph_scc(want_comp=True)
        assert scc_fields(s) == e["scc"]
        assert s.trimmed == e["states"] and s.nontrivial == 0  # acyclic: the trimming alone, no colouring round
        assert np.array_equal(s.comp, np.arange(e["states"], dtype=np.uint32))
        assert mc.graph_shape()["cyclic_states"] == 0


def test_query_between_steps_is_that_of_the_truncated_graph():
    name, k = "n3_v1_e1_r3", 6
    ls = LIVE[name]["level_starts"]
    n = ls[k + 1]  # init() + k steps: levels 1 .. k + 1 stand, the parents of levels 1 .. k have their edges
    edges = np.array([x for x in FULL[name]["edges"] if x[0] < ls[k]], dtype=np.int64)
    src, dst = edges[:, 0], edges[:, 2]
    inv = inv_values(R.Config(max_restart=3, **FULL_KW[name]), FULL[name]["states"][:n])
    lv = np_levels(n, src, dst)
    with make(name) as mc:
        mc.set_graph_keep()
        mc.init()
        for _ in range(k):
            mc.step()
        want, within = np_live_query(n, src, dst, targets_of(inv, 2, True), lv)
        r = mc.graph_eventually("RaftCanCommt", want_within=True)
        got = live_fields(mc, r, mc.graph_eventually_levels())
        del want["within_sha256"]
        assert got == want and np.array_equal(r.within, within)
        assert r.avoiders > LIVE[name]["queries"]["RaftCanCommt=TRUE"]["avoiders"] - (LIVE[name]["states"] - n)
        s = mc.graph_scc()
        assert (s.trimmed, s.nontrivial, s.components) == (n, 0, n)


# ---- b / c. imported graphs ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def imc():
    with raftmc.ModelChecker(raftmc.ModelConfig(n_servers=2, n_vals=1, max_election=1, max_restart=1)) as mc:
        mc.set_graph_keep()
        yield mc


def check_live(mc, n, src, dst, inv, queries=((0, True, None, True),)):
    """Each (bit, value, source bit or None, source value) against live_ref; must is inside can_reach, within >= dist."""
    src, dst, inv = np.asarray(src, dtype=np.uint32), np.asarray(dst, dtype=np.uint32), np.asarray(inv, dtype=np.uint16)
    mc.graph_import(n, src, dst, inv)
    out = []
    for b, value, sb, svalue in queries:
        name = raftmc.INVARIANT_BY_BIT[b]
        sname = None if sb is None else raftmc.INVARIANT_BY_BIT[sb]
        want, within = np_live_query(n, src, dst, targets_of(inv, b, value),
                                     source=None if sb is None else targets_of(inv, sb, svalue))
        del want["within_sha256"]
        r = mc.graph_eventually(name, value, source=sname, source_value=svalue, want_within=True)
        got = live_fields(mc, r, mc.graph_eventually_levels())
        assert got == want, (b, value, sb, svalue)
        assert np.array_equal(r.within, within)
        assert (r.states, r.edges, r.self_edges) == (n, len(src), int((src == dst).sum()))
        assert r.rounds == (r.max_within + 1 if r.targets else 0)
        assert r.must + r.avoiders == n
        paths = (got["avoid_path"], got.get("source_path"))
        dist = mc.graph_reach(name, value, want_dist=True).dist  # (ends the liveness query: the paths are read already)
        m = within != UNSET
        assert (dist[m] != UNSET).all() and (within[m] >= dist[m]).all()
        out.append((r, paths))
    return out


def check_scc(mc, n, src, dst, import_it=True):
    src, dst = np.asarray(src, dtype=np.uint32), np.asarray(dst, dtype=np.uint32)
    if import_it:
        mc.graph_import(n, src, dst, np.zeros(n, dtype=np.uint16))
    label = np_scc(n, src, dst)
    s = mc.graph_scc(want_comp=True)
    assert s.comp.dtype == np.uint32 and np.array_equal(s.comp, label)
    assert scc_fields(s) == scc_summary(label)
    cyc = mc.graph_shape()["cyclic_states"]
    assert s.nontrivial_states <= cyc and (s.nontrivial_states == 0) == (cyc == 0)
    assert s.trimmed <= n - s.nontrivial_states
    if s.nontrivial == 0:
        assert s.trimmed == n  # no cycle: the trimming ends it
    return s


def test_live_one_state_no_edge(imc):
    (r, paths), = check_live(imc, 1, [], [], [0])  # empty T: a terminal avoider
    assert (r.must, r.avoiders, r.avoid_terminal, r.first_avoid, r.init_within, r.rounds) == (0, 1, 1, 0, None, 0)
    assert paths[0] == dict(gids=[0], loop_at=None)
    (r, paths), = check_live(imc, 1, [], [], [1])  # full T
    assert (r.must, r.avoiders, r.first_avoid, r.init_within, r.max_within, r.rounds) == (1, 0, None, 0, 0, 1)
    assert r.within.tolist() == [0] and paths[0] is None


def test_live_self_edges_only(imc):
    n = 5
    (r, _), = check_live(imc, n, list(range(n)) + [2], list(range(n)) + [2], [1, 0, 1, 0, 0])
    assert r.within.tolist() == [0, UNSET, 0, UNSET, UNSET]
    assert (r.must, r.avoiders, r.avoid_terminal, r.first_avoid, r.self_edges) == (2, 3, 3, 1, 6)


def test_live_chain_of_1000(imc):
    n = 1000
    inv = np.zeros(n, dtype=np.uint16)
    inv[n - 1] = 1
    (r, _), = check_live(imc, n, np.arange(n - 1), np.arange(1, n), inv)
    assert np.array_equal(r.within, np.arange(n - 1, -1, -1, dtype=np.uint32))
    assert (r.rounds, r.max_within, r.init_within, r.must) == (1000, 999, 999, 1000)


def test_live_diamond_takes_the_longer_branch(imc):
    # 0 -> 1 -> 5 (branch of length 1 below the top's edge) and 0 -> 2 -> 3 -> 4 -> 5 (length 3); 5 is the target
    src, dst = [0, 1, 0, 2, 3, 4], [1, 5, 2, 3, 4, 5]
    (r, _), = check_live(imc, 6, src, dst, [0, 0, 0, 0, 0, 1])
    assert r.within.tolist() == [4, 1, 3, 2, 1, 0] and r.init_within == 4
    assert imc.graph_reach("Inv", True, want_dist=True).dist.tolist()[0] == 2


def test_live_target_whose_successors_are_attracted_enters_no_second_frontier(imc):
    # targets 1 and 2: 1 -> 2, 1 -> 3, 3 -> 2, so 1's counter reaches zero in round 2; 0 -> 1 must not be counted twice,
    # and 0's other edge 0 -> 4 -> 1 makes a second decrement of 0 by a re-entered 1 visible as a wrong within
    src, dst = [1, 1, 3, 0, 0, 4], [2, 3, 2, 1, 4, 1]
    (r, _), = check_live(imc, 5, src, dst, [0, 1, 1, 0, 0])
    assert r.within.tolist() == [2, 0, 0, 1, 1] and (r.targets, r.must, r.rounds) == (2, 5, 3)


def test_live_duplicate_edges_and_self_edge(imc):
    # 1 has three duplicate edges to the target 0 and nothing else; 2 has a self-edge and one edge to 0
    src, dst = [1, 1, 1, 2, 2], [0, 0, 0, 2, 0]
    (r, _), = check_live(imc, 3, src, dst, [1, 0, 0])
    assert r.within.tolist() == [0, 1, 1] and r.avoiders == 0


def test_live_sink_below_a_targets_predecessor(imc):
    # 0 -> 1 (target) and 0 -> 2 (a sink that is no target): 0 is an avoider, its witness ends in 2
    (r, paths), = check_live(imc, 3, [0, 0], [1, 2], [0, 1, 0])
    assert r.within.tolist() == [UNSET, 0, UNSET]
    assert (r.avoiders, r.avoid_terminal, r.first_avoid, r.init_within) == (2, 1, 0, None)
    assert paths[0] == dict(gids=[0, 2], loop_at=None)


def test_live_two_cycle_with_an_exit_is_a_lasso(imc):
    # 0 -> 1 <-> 2, 2 -> 3 (target): 0, 1, 2 can stay on the cycle forever; from 0 the lasso closes at index 1
    (r, paths), = check_live(imc, 4, [0, 1, 2, 2], [1, 2, 1, 3], [0, 0, 0, 1])
    assert r.within.tolist() == [UNSET, UNSET, UNSET, 0]
    assert (r.must, r.avoiders, r.avoid_terminal) == (1, 3, 0)
    assert paths[0] == dict(gids=[0, 1, 2], loop_at=1)
    assert imc.graph_eventually("Inv").avoiders == 3
    assert imc.graph_avoid_path(2) == ([2, 1], 0) and imc.graph_avoid_path(1) == ([1, 2], 0)


def test_live_fan_in_and_fan_out_of_5000(imc):
    n = 5001
    inv = np.zeros(n, dtype=np.uint16)
    inv[0] = 1
    (r, _), = check_live(imc, n, np.arange(1, n), np.zeros(n - 1, dtype=np.uint32), inv)  # 5,000 states -> one target
    assert (r.must, r.max_within, r.rounds) == (n, 1, 2)
    inv = np.ones(n, dtype=np.uint16)
    inv[0] = 0
    (r, _), = check_live(imc, n, np.zeros(n - 1, dtype=np.uint32), np.arange(1, n), inv)  # one state -> 5,000 targets
    assert (r.must, r.init_within, r.targets) == (n, 1, 5000)
    inv[n - 1] = 0  # one of the 5,000 is no target and a sink: the hub can avoid
    (r, paths), = check_live(imc, n, np.zeros(n - 1, dtype=np.uint32), np.arange(1, n), inv)
    assert (r.avoiders, r.avoid_terminal, paths[0]) == (2, 1, dict(gids=[0, n - 1], loop_at=None))


def test_live_leads_to_holds_and_fails(imc):
    # 0 -> 1 -> 2 (target), 3 -> 4 (sink, no target); bit 1 marks the source set
    src, dst = [0, 1, 3], [1, 2, 4]
    holds = [2, 2, 1, 0, 0]  # sources 0, 1: disjoint from the avoiders 3, 4
    (r, paths), = check_live(imc, 5, src, dst, holds, queries=((0, True, 1, True),))
    assert (r.sources, r.source_avoiders, r.first_source_avoid, r.avoiders, paths[1]) == (2, 0, None, 2, None)
    fails = [2, 0, 1, 2, 0]  # sources 0, 3
    (r, paths), = check_live(imc, 5, src, dst, fails, queries=((0, True, 1, True),))
    assert (r.sources, r.source_avoiders, r.first_source_avoid, r.first_source_avoid_level) == (2, 1, 3, 1)
    assert paths[1] == dict(gids=[3, 4], loop_at=None)


@pytest.mark.parametrize("m", [2200, 4000, 8000])
def test_live_random_graph(imc, m):
    rng = np.random.default_rng(20250600 + m)
    n = 2000
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    inv = (rng.integers(0, 2, n) | (rng.integers(0, 8, n) == 0) << 2).astype(np.uint16)  # bit 0: half; bit 2: an eighth
    err = rng.integers(0, 8, n) == 0  # an eighth raise the evaluation error of invariant 0: in neither of its sets
    inv[err] = (inv[err] & ~np.uint16(1)) | np.uint16(1 << 8)
    # bit 1 is never set: "NoSplitVote = TRUE" is the empty target set and "= FALSE" the full one
    got = check_live(imc, n, src, dst, inv, queries=((0, True, None, True), (0, False, None, True), (2, True, 0, True),
                                                      (2, True, 0, False), (1, True, None, True), (1, False, None, True)))
    empty, full = got[4][0], got[5][0]
    assert (empty.targets, empty.must, empty.rounds, empty.first_avoid) == (0, 0, 0, 0)
    assert (full.targets, full.must, full.avoiders, full.max_within, full.first_avoid) == (n, n, 0, 0, None)
    assert any(r.avoiders and r.must > r.targets for r, _ in got[:4])


def test_scc_single_state_and_self_edges(imc):
    s = check_scc(imc, 1, [], [])
    assert (s.components, s.trimmed, s.largest) == (1, 1, 1)
    s = check_scc(imc, 5, [0, 1, 2, 3, 4, 2], [0, 1, 2, 3, 4, 2])
    assert (s.components, s.nontrivial, s.trimmed) == (5, 0, 5)


def test_scc_chain_cycle_and_two_way_chain_of_1000(imc):
    n = 1000
    a = np.arange(n - 1)
    s = check_scc(imc, n, a, a + 1)
    assert (s.components, s.trimmed, s.nontrivial) == (n, n, 0)
    s = check_scc(imc, n, np.arange(n), (np.arange(n) + 1) % n)
    assert (s.components, s.nontrivial, s.largest, s.trimmed) == (1, 1, n, 0)
    s = check_scc(imc, n, np.concatenate([a, a + 1]), np.concatenate([a + 1, a]))
    assert (s.components, s.nontrivial, s.largest) == (1, 1, n)


def test_scc_small_shapes(imc):
    # two 3-cycles joined one way
    s = check_scc(imc, 6, [0, 1, 2, 2, 3, 4, 5], [1, 2, 0, 3, 4, 5, 3])
    assert (s.components, s.nontrivial, s.nontrivial_states, s.largest) == (2, 2, 6, 3)
    assert s.comp.tolist() == [0, 0, 0, 3, 3, 3]
    # a figure-eight through the shared state 2
    s = check_scc(imc, 5, [0, 1, 2, 2, 3, 4], [1, 2, 0, 3, 4, 2])
    assert (s.components, s.largest) == (1, 5)
    # duplicated edges
    s = check_scc(imc, 4, [0, 0, 1, 1, 1, 2, 2], [1, 1, 0, 0, 2, 3, 3])
    assert s.comp.tolist() == [0, 0, 2, 3]
    # a cycle listed in descending gid order, behind a chain whose gids are larger: the label is the smallest gid, which
    # is not where a max-gid propagation roots the component
    s = check_scc(imc, 7, [4, 3, 2, 1, 6, 5], [3, 2, 1, 4, 5, 4])
    assert s.comp.tolist() == [0, 1, 1, 1, 1, 5, 6]


def test_scc_hub_of_in_degree_5000_with_one_edge_back(imc):
    n = 5001
    src = np.concatenate([np.arange(1, n), [0]])
    dst = np.concatenate([np.zeros(n - 1, dtype=np.int64), [17]])
    s = check_scc(imc, n, src, dst)
    assert (s.components, s.nontrivial, s.nontrivial_states, s.largest) == (n - 1, 1, 2, 2)
    assert s.comp[17] == 0 and s.comp[0] == 0


@pytest.mark.parametrize("m", [2200, 6000])
def test_scc_random_graph(imc, m):
    rng = np.random.default_rng(20250700 + m)
    n = 2000
    s = check_scc(imc, n, rng.integers(0, n, m), rng.integers(0, n, m))
    if m == 6000:
        assert s.largest > n // 2  # one giant component
    else:
        assert s.nontrivial >= 1 and s.largest < n // 2


# ---- d. state rules ----------------------------------------------------------------------------------------------
def test_ordering_and_errors():
    name = "n3_v1_e1_r3"
    calls = [lambda m: m.graph_eventually("RaftCanCommt"), lambda m: m.graph_scc(), lambda m: m.graph_eventually_levels(),
             lambda m: m.graph_avoid_path(0)]
    with make(name) as mc:  # keep off
        mc.run()
        for f in calls:
            with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
                f(mc)
    with make(name) as mc:
        mc.set_graph_keep()
        for f in calls:  # on, nothing kept yet
            with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
                f(mc)
        mc.init()
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.graph_avoid_path(0)  # a graph, no query yet
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.graph_eventually_levels()
        r0 = mc.graph_eventually("RaftCanCommt")  # Init alone: a terminal avoider
        assert (r0.states, r0.avoiders, r0.avoid_terminal) == (1, 1, 1) and mc.graph_avoid_path(0) == ([0], None)
        mc.run()
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.graph_avoid_path(0)  # the graph has grown since the query
        r = mc.graph_eventually("RaftCanCommt", want_within=True)  # the CSR is rebuilt for the grown graph
        must = int(np.flatnonzero(r.within != UNSET)[0])
        with pytest.raises(raftmc.RmcError, match="RMC_E_ARG"):
            mc.graph_avoid_path(must)  # no avoider
        with pytest.raises(raftmc.RmcError, match="RMC_E_ARG"):
            mc.graph_avoid_path(r.states)  # no state
        with pytest.raises(ValueError):
            mc.graph_eventually("RaftCanCommt", source="NoSuchInvariant")  # (as graph_reach: the binding's own lookup)
        s = mc.graph_scc()
        gids, at = mc.graph_avoid_path(r.first_avoid)  # the components leave the query standing
        mc.graph_reach("RaftCanCommt")
        with pytest.raises(raftmc.RmcError, match="RMC_E_STATE"):
            mc.graph_avoid_path(r.first_avoid)  # a reachability query took the distances back
    with make(name) as fresh:
        fresh.set_graph_keep()
        fresh.run()
        f = fresh.graph_eventually("RaftCanCommt", want_within=True)
        assert np.array_equal(f.within, r.within) and (f.must, f.first_avoid) == (r.must, r.first_avoid)
        assert fresh.graph_avoid_path(f.first_avoid) == (gids, at)
        assert scc_fields(fresh.graph_scc()) == scc_fields(s)


# ---- e. launcher ---------------------------------------------------------------------------------------------------
def _normal(out):
    out = re.sub(r"\d{4}-\d\d-\d\d \d\d:\d\d:\d\d", "<time>", out)
    out = re.sub(r"\(\d+ d?s/min\)", "(<rate>)", out)
    out = re.sub(r"Finished in [\d.]+s", "Finished in <s>", out)
    return re.sub(r"(?m)^GPU: .*$", "GPU: <rate>", out)


def _states_of(block):
    """the printed behaviour as a list of (header, state lines), the msgs continuation lines joined"""
    out = []
    for l in block:
        if re.match(r"State \d+: ", l):
            out.append((l, []))
        elif l.startswith("   [") and out:
            out[-1][1][-1] += " " + l.strip()
        elif l and out:
            out[-1][1].append(l)
    return [(h, [x.replace(",  [", ", [") for x in ls]) for h, ls in out]


def test_launcher_eventually_and_scc(tmp_path):
    from test_host import LAUNCHER, cfg_text
    name = "n3_v1_e1_r3"
    e = LIVE[name]
    q = e["queries"]["RaftCanCommt=TRUE"]
    (tmp_path / "Raft.cfg").write_text(cfg_text(E=1, R=3, servers="s1, s2, s3", vals="v1"))
    env = dict(os.environ, RMC_SKIP_SPEC_CHECK="1")
    base = [LAUNCHER, "-deadlock", "-config", str(tmp_path / "Raft.cfg")]
    tla = str(tmp_path / "Raft.tla")
    plain = subprocess.run(base + [tla], capture_output=True, text=True, env=env, timeout=120)
    r = subprocess.run(base + ["-eventually", "RaftCanCommt", "-scc", tla], capture_output=True, text=True, env=env, timeout=120)
    assert plain.returncode == r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("Inevitability of ")]
    end = [i for i, l in enumerate(lines) if l.startswith("The state graph has ")]
    assert len(at) == 1 and len(end) == 1 and at[0] < end[0]
    init = "Init can avoid it" if q["init_within"] is None else f"Init: {q['init_within']} steps"
    assert lines[at[0]] == (
        f"Inevitability of RaftCanCommt = TRUE: {q['targets']} of {e['states']} distinct states satisfy it, {q['must']} must "
        f"reach one (latest: {q['max_within']} steps, {init}), {q['avoiders']} can avoid it forever (first at depth "
        f"{q['first_avoid_level']}; {q['avoid_terminal']} of them end where no step leads out).")
    s = e["scc"]
    assert lines[end[0]] == (f"The state graph has {s['components']} strongly connected components: {s['nontrivial']} of more "
                             f"than one state ({s['nontrivial_states']} states, the largest {s['largest']}).")
    # Init can avoid a commit (an election may never come), so the property fails and the behaviour is printed: the
    # BFS-tree path to the first avoider (Init itself), then the avoid walk
    assert q["init_within"] is None and q["first_avoid"] == 0
    block = lines[at[0] + 1:end[0]]
    assert block[0] == "Error: Temporal properties were violated."
    assert block[1] == "Error: The following behavior constitutes a counter-example:"
    path = q["avoid_path"]
    shown = _states_of(block[2:])
    closing = shown[-1][0] if re.match(r"State \d+: Stuttering", shown[-1][0]) else [l for l in block if l.startswith("Back to state")][-1]
    if path["loop_at"] is None:
        assert closing == f"State {len(path['gids']) + 1}: Stuttering" and block[-1] == closing
        shown = shown[:-1]
    else:
        assert closing.startswith(f"Back to state {path['loop_at'] + 1}: <") and block[-1] == closing
    assert len(shown) == len(path["gids"]) and shown[0][0] == "State 1: <Initial predicate>"
    for (_h, got), g in zip(shown, path["gids"]):
        assert got == render_state(FULL[name]["states"][g], ["s1", "s2", "s3"], ["v1"]), g
    # without the flags: the parent's output; with them, the same lines around the new ones, and the same exit code
    rest = lines[:at[0]] + lines[end[0] + 1:]
    assert _normal("\n".join(rest)) == _normal("\n".join(plain.stdout.splitlines()))
    assert "Inevitability" not in plain.stdout and "The state graph has" not in plain.stdout


def test_launcher_leadsto(tmp_path):
    """A leads-to that fails away from Init: the BFS-tree path to the first source avoider, then the walk; and one that
    holds (no source state), which prints its line alone."""
    from test_host import LAUNCHER, cfg_text
    name = "n3_v1_e1_r3"
    e = LIVE[name]
    (tmp_path / "Raft.cfg").write_text(cfg_text(E=1, R=3, servers="s1, s2, s3", vals="v1"))
    env = dict(os.environ, RMC_SKIP_SPEC_CHECK="1")
    r = subprocess.run([LAUNCHER, "-deadlock", "-config", str(tmp_path / "Raft.cfg"), "-leadsto", "RaftCanCommt", "CommitAll",
                        "-leadsto", "ExistLeaderAndCandidate", "RaftCanCommt", str(tmp_path / "Raft.tla")],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    at = [i for i, l in enumerate(lines) if l.startswith("Leads-to ")]
    assert len(at) == 2
    q = e["queries"]["RaftCanCommt=TRUE~>CommitAll=TRUE"]
    assert lines[at[0]] == (
        f"Leads-to RaftCanCommt = TRUE ~> CommitAll = TRUE: {q['sources']} of {e['states']} distinct states satisfy the first, "
        f"{q['source_avoiders']} of them can avoid the second forever (first at depth {q['first_source_avoid_level']}); "
        f"{q['targets']} of {e['states']} distinct states satisfy it, {q['must']} must reach one (latest: {q['max_within']} steps, "
        f"Init can avoid it), {q['avoiders']} can avoid it forever (first at depth {q['first_avoid_level']}; "
        f"{q['avoid_terminal']} of them end where no step leads out).")
    block = lines[at[0] + 1:at[1]]
    assert block[:2] == ["Error: Temporal properties were violated.",
                         "Error: The following behavior constitutes a counter-example:"]
    path = q["source_path"]
    assert path["loop_at"] is None and path["gids"][0] == q["first_source_avoid"]
    shown = _states_of(block[2:])
    stem = q["first_source_avoid_level"] - 1  # states before the first source avoider
    assert len(shown) == stem + len(path["gids"]) + 1 and shown[0][0] == "State 1: <Initial predicate>"
    assert shown[-1] == (f"State {stem + len(path['gids']) + 1}: Stuttering", []) and block[-1] == shown[-1][0]
    for (h, got), g in zip(shown[stem:-1], path["gids"]):
        assert re.match(r"State \d+: <\w+ line \d+|State \d+: <\w+\(", h), h
        assert got == render_state(FULL[name]["states"][g], ["s1", "s2", "s3"], ["v1"]), g
    q2 = e["queries"]["ExistLeaderAndCandidate=TRUE~>RaftCanCommt=TRUE"]
    assert (q2["sources"], q2["source_avoiders"]) == (0, 0)
    assert lines[at[1]].startswith(f"Leads-to ExistLeaderAndCandidate = TRUE ~> RaftCanCommt = TRUE: 0 of {e['states']} distinct "
                                   "states satisfy the first, 0 of them can avoid the second forever; ")
    assert not lines[at[1] + 1].startswith("Error:")
