"""Graph mode (rmc_set_graph; raftmc -dump) without a device: the golden fixture (tests/golden/graph.json and
graph_full.json.gz, tests/golden/make_golden_graph.py) against the level and coverage fixtures of the same
configurations, its generator rerun on small ones, the test's dump and dot renderers on Init, the library's
exports and the launcher's refusals."""
import ctypes
import gzip
import json
import os
import subprocess
import sys

import pytest

import raftmc
from conftest import GOLDEN, ROOT, has_gpu
from graph_render import dot_label, dot_text, dump_text
from tla_render import render_state

sys.path.insert(0, GOLDEN)
import make_golden_graph as MG  # noqa: E402

import raft_ref as R  # noqa: E402

LAUNCHER = os.path.join(ROOT, "tla-raft_amd", "build", "raftmc")
TWIN = "noinv_seeded_n3_v1_e2_r3"
ERRORS = {"seeded_n3_v1_e2_r3": "invariant", "sb_n3_v1_e2_r3": "assert", "deadlock_n3_v1_e1_r3": "deadlock",
          "cpl_n3_v2_e1_r3": "eval_error"}


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


GRAPH = load("graph.json")
COVERAGE = load("coverage.json")
with gzip.open(os.path.join(GOLDEN, "graph_full.json.gz")) as _f:
    FULL = json.load(_f)


def test_fixture_holds_the_coverage_configurations_and_the_twin():
    assert list(GRAPH) == list(COVERAGE) + [TWIN] == list(MG.CONFIGS) and len(GRAPH) == 13
    assert {n: GRAPH[n]["verdict"] for n in ERRORS} == ERRORS
    assert all(GRAPH[n]["verdict"] == "ok" for n in GRAPH if n not in ERRORS)
    assert list(FULL) == list(MG.FULL) == ["n2_v1_e2_r3", "n3_v1_e1_r3"]
    assert all(os.path.getsize(os.path.join(GOLDEN, f)) < (1 << 20) for f in ("graph.json", "graph_full.json.gz"))


@pytest.mark.parametrize("name", list(COVERAGE))
def test_fixture_agrees_with_the_level_and_coverage_fixtures(name):
    e, c = GRAPH[name], COVERAGE[name]
    g = load(c["levels_file"])[name]
    assert e["levels_file"] == c["levels_file"] and e["verdict"] == g["verdict"] == c["verdict"]
    assert e["states"] == g["distinct"]
    assert sum(e["by_action"]) == e["edges"] == e["edges_per_level"][-1]
    assert e["edges_per_level"] == sorted(e["edges_per_level"])
    if e["verdict"] == "ok":
        assert e["edges"] == g["generated"] - 1
        assert e["by_action"] == c["generated"]
        per = e["edges_per_level"]
        assert [b - a for a, b in zip([0] + per, per)] == g["gen_per_level"]
    else:
        # TLC counts a whole sub-action batch before it fingerprints any of it; the edges stop at the erring successor
        assert e["edges"] <= g["generated"] - 1
        assert all(a <= b for a, b in zip(e["by_action"], c["generated"]))
        if e["verdict"] in ("assert", "deadlock"):
            assert e["by_action"] == c["generated"]


def test_the_twin_is_what_continue_searches():
    cont = load("continue.json")["seeded_n3_v1_e2_r3"]
    e = GRAPH[TWIN]
    assert (e["verdict"], e["states"], e["edges"]) == ("ok", cont["distinct"], cont["generated"] - 1)
    assert e["by_action"] == cont["coverage"]["generated"]


@pytest.mark.parametrize("name", list(FULL))
def test_full_lists_match_their_entry_and_every_first_edge_is_a_tree_edge(name):
    e, edges, states = GRAPH[name], FULL[name]["edges"], FULL[name]["states"]
    assert (len(states), len(edges)) == (e["states"], e["edges"])
    assert MG.edges_digest(edges) == e["edges_sha256"] and MG.states_digest(states) == e["states_sha256"]
    assert MG.states_digest(states[::MG.SAMPLE]) == e["states_sample_sha256"]
    first = {}
    for src, _key, dst in edges:
        first.setdefault(dst, src)
    assert sorted(first) == list(range(0 if 0 in first else 1, len(states)))
    assert all(first[d] < d for d in first if d > 0)
    assert [s for s, _k, _d in edges] == sorted(s for s, _k, _d in edges)
    want = MG.SPOT[name]
    assert (len(states), len(edges)) + MG.shape(len(states), edges) + (e["edges_sha256"][:16],) == want


@pytest.mark.parametrize("name", ["n3_v1_e1_r3", "sb_n3_v1_e2_r3", "deadlock_n3_v1_e1_r3"])
def test_generator_reproduces_the_committed_entry(name):
    got_name, e, full = MG.entry(name)
    assert got_name == name and e == GRAPH[name]
    if name in FULL:
        assert full == FULL[name]


@pytest.mark.parametrize("name", list(ERRORS))
def test_error_entries_reach_only_delivered_states(name):
    """On an error every dst is below the reported `distinct`, and every state but Init has a tree edge."""
    _src, kw = MG.CONFIGS[name]
    verdict, states, edges, per_level = MG.graph_bfs(R.Config(max_restart=3, **kw))
    g = load(GRAPH[name]["levels_file"])[name]
    assert verdict == GRAPH[name]["verdict"] and len(states) == g["distinct"] == GRAPH[name]["states"]
    assert all(d < len(states) for _s, _k, d in edges) and per_level == GRAPH[name]["edges_per_level"]
    first = {}
    for src, _key, dst in edges:
        first.setdefault(dst, src)
    assert all(d in first and first[d] < d for d in range(1, len(states)))


def test_renderers_agree_with_tla_render_on_init():
    st = R.state_to_json(R.init_state(R.Config(n=2, V=1, max_election=2, max_restart=3)))
    lines = render_state(st, ["s1", "s2"], ["v1"])
    assert dump_text([st], ["s1", "s2"], ["v1"]) == "State 1:\n" + "\n".join(lines) + "\n\n"
    label = "\\n".join(l.replace("\\", "\\\\") for l in lines)
    assert dot_label(st, ["s1", "s2"], ["v1"]) == label and label.startswith("/\\\\ votedFor = (s1 :> None @@ s2 :> None)")
    assert dot_text([st], [(0, 1 << 16, 0)], ["s1", "s2"], ["v1"], True).splitlines() == [
        "strict digraph DiskGraph {", "nodesep=0.35;", "subgraph cluster_graph {", 'color="white";',
        f'1 [label="{label}",style = filled]', '1 -> 1 [label="UpdateTerm",color="black",fontcolor="black"];', "}", "}"]
    assert 'label=""' in dot_text([st], [(0, 1 << 16, 0)], ["s1", "s2"], ["v1"], False)


def test_library_exports_set_graph_within_abi_5():
    lib = raftmc.load_library()
    assert hasattr(lib, "rmc_set_graph") and lib.rmc_abi_version() == 5
    assert raftmc.ERRORS[-8] == "RMC_E_SINK"
    assert ctypes.sizeof(raftmc._GraphSink) == 32
    header = open(os.path.join(ROOT, "include", "rmc.h")).read()
    assert "#define RMC_ABI_VERSION 5" in header and "#define RMC_E_SINK -8" in header


@pytest.mark.parametrize("args,word", [
    (["-dump"], "-dump"),
    (["-dump", "dot"], "-dump dot"),
    (["-dump", "dot,colorize", "g", "Raft.tla"], "colorize"),
    (["-dump", "dot,actionlabels,snapshot", "g", "Raft.tla"], "snapshot"),
    (["-dump", "g", "-simulate", "Raft.tla"], "-simulate"),
    (["-dump", "dot", "g", "-recover", "states", "Raft.tla"], "-recover"),
    (["-dump", "g", "-gpus", "2", "Raft.tla"], "-gpus"),
])
def test_launcher_dump_usage_errors(args, word):
    """Refused before any file is read or a device touched."""
    r = subprocess.run([LAUNCHER] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 150, r.stdout + r.stderr
    first = r.stderr.splitlines()[0]
    assert word in first and "unsupported option" not in first
    assert r.stdout == ""
    if len(args) > 2:
        assert "usage: raftmc" in r.stderr and "-dump" in r.stderr


def test_launcher_dump_reaches_device_creation(tmp_path):
    """-dump and -dump dot,actionlabels are options the launcher knows: without a device the run ends where
    every run does, at the creation of the checker."""
    if has_gpu():
        pytest.skip("the no-device path needs a machine without a GPU")
    from test_host import cfg_text
    (tmp_path / "Raft.cfg").write_text(cfg_text(E=2, R=3, servers="s1, s2", vals="v1"))
    env = dict(os.environ, RMC_SKIP_SPEC_CHECK="1")
    for extra in (["-dump", str(tmp_path / "g")], ["-dump", "dot,actionlabels", str(tmp_path / "g")]):
        r = subprocess.run([LAUNCHER, "-deadlock", "-config", str(tmp_path / "Raft.cfg")] + extra +
                           [str(tmp_path / "Raft.tla")], capture_output=True, text=True, env=env, timeout=120)
        assert r.returncode == 75, r.stdout + r.stderr
        assert "Error: could not start the GPU model checker" in r.stdout and "unsupported option" not in r.stderr
