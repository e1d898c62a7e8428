"""Chunk look-ahead on one GPU (RMC_LOOKAHEAD, rmc_engine.hip step_single): within a level, split chunk
k + 1 is expanded on its own stream into a second staging set while chunk k probes and commits.

Every case splits every chunk (RMC_SPLIT_MIN=1), drives the levels from the host (device_levels=1) and
takes chunks of 6000 successor slots: 64-70 parents each, so the wide levels have from 3 to several
hundred chunks and every chunk but a level's last looks ahead.  The results must be the golden ones
(tests/golden/, from oracle/) and equal to those of the single-stream order (RMC_LOOKAHEAD=0)."""
import json
import os

import pytest

import raftmc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def load(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


LEVELS = load("levels.json")
TRACES = load("traces.json")
LEVELS_BF = load("levels_bf.json")
LEVELS_ERR = load("levels_errors.json")
TRACES_ERR = load("traces_errors.json")

CHUNK = 6000
KW = dict(device_levels=1, chunk_successors=CHUNK)
PH_HASH = 1  # the expansion's phase (rmc_engine.hip Phase)


# the two helpers of tests/test_gpu.py
def spec_of(g):
    if g.get("become_follower"):
        return raftmc.SPEC_BECOME_FOLLOWER
    if g.get("variant"):
        return {"split_brain": raftmc.SPEC_SPLIT_BRAIN, "commit_past_log": raftmc.SPEC_COMMIT_PAST_LOG}[g["variant"]]
    return raftmc.SPEC_SEEDED if g["seeded"] else raftmc.SPEC_RAFT


def run_cfg(g, **kw):
    mc = raftmc.ModelChecker(raftmc.ModelConfig(
        n_servers=g["n"], n_vals=g["V"], max_election=g["E"], max_restart=g["R"],
        invariants=tuple(g["invariants"]), check_deadlock=g["check_deadlock"],
        spec_variant=spec_of(g), **kw))
    res = mc.run()
    return mc, res


def check_levels(g, res):
    assert res.status == {"ok": "done"}.get(g["verdict"], g["verdict"])
    assert res.generated == g["generated"] and res.distinct == g["distinct"]
    if g["verdict"] == "ok":
        assert res.depth == g["depth"]
        assert [ls.new_states for ls in res.levels if ls.new_states] == g["levels"]
        assert [ls.generated for ls in res.levels[1:]] == g["gen_per_level"]
        assert res.queue == 0
    else:
        assert res.trace_len == g["trace_len"]
        assert res.queue == g["queue_left"]
        if g["verdict"] == "invariant":
            assert res.violated == g["violated"]


def trace_of(mc):
    return [(list(k) if k else None, st) for k, st in mc.trace()]


def golden_trace(t):
    return [(e["key"], e["state"]) for e in t["steps"]]


def level_counts(res):
    return [(ls.expanded, ls.generated, ls.new_states, ls.self_loops, ls.new_bytes) for ls in res.levels]


def chunk_parents(g):
    """Parents per chunk (rmc_engine.hip setup: Gcap / maxsucc; maxsucc = Spec::MAXS of one message round
    for n <= 3, two above)."""
    n = g["n"]
    maxsucc = (64 if n <= 3 else 128) + n * (4 + g["V"] + n - 1)
    return max(CHUNK, 64 * maxsucc) // maxsucc


@pytest.fixture
def split_all(monkeypatch):
    monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    return monkeypatch


COUNT_CASES = ["n3_v2_e1_r3", "n3_v1_e2_r3", "n4_v1_e1_r3", "n5_v1_e1_r3", "seeded_n3_v2_e2_r3", "seeded_n3_v1_e2_r3"]


@pytest.mark.parametrize("name", COUNT_CASES)
def test_lookahead_counts_and_traces_equal_single_stream(name, split_all):
    """Look-ahead on and off: both the golden run, per-level counters equal between the two, and the
    golden counterexample where there is one."""
    g = LEVELS[name]
    assert max(g["levels"]) >= 3 * chunk_parents(g)  # the widest level has at least 3 chunks
    per_mode = {}
    for mode in ("1", "0"):
        split_all.setenv("RMC_LOOKAHEAD", mode)
        mc, res = run_cfg(g, **KW)
        check_levels(g, res)
        per_mode[mode] = level_counts(res)
        if name in TRACES:
            assert trace_of(mc) == golden_trace(TRACES[name])
        mc.close()
    assert per_mode["1"] == per_mode["0"]


@pytest.mark.parametrize("name", ["bf_n4_v1_e1_r3", "bf_n3_v1_e2_r3"])
def test_lookahead_sparse_layout(name, split_all):
    """The chunks whose winners the items commit does not take (k_insert_winners + k_commit_split, no
    dense slot offsets): the BecomeFollower variant."""
    split_all.setenv("RMC_LOOKAHEAD", "1")
    g = LEVELS_BF[name]
    mc, res = run_cfg(g, **KW)
    check_levels(g, res)
    mc.close()


@pytest.mark.parametrize("name", ["sb_n3_v2_e2_r3", "sb_n3_v1_e2_r3", "cpl_n3_v2_e1_r3", "sb_n3_v1_e3_r3"])
def test_lookahead_errors_and_rerun(name, split_all):
    """An Assert (found by an expansion), an evaluation error and an invariant violation (found by a
    commit) while the next chunk's expansion is in flight: TLC's verdict, counters and counterexample;
    after reset() the same checker gives the same result again, so the dropped expansion left
    nothing in its staging set."""
    split_all.setenv("RMC_LOOKAHEAD", "1")
    g = LEVELS_ERR[name]
    mc, res = run_cfg(g, **KW)
    first = (res.status, res.generated, res.distinct, res.depth, res.queue, res.trace_len, res.violated)
    check_levels(g, res)
    assert [ls.new_states for ls in res.levels if ls.new_states][:len(g["levels"]) - 1] == g["levels"][:-1]
    counts = level_counts(res)
    assert trace_of(mc) == golden_trace(TRACES_ERR[name])
    mc.reset()
    res = mc.run()
    check_levels(g, res)
    assert (res.status, res.generated, res.distinct, res.depth, res.queue, res.trace_len, res.violated) == first
    assert level_counts(res) == counts
    assert trace_of(mc) == golden_trace(TRACES_ERR[name])
    mc.close()


@pytest.mark.parametrize("name", ["n3_v2_e1_r3", "n3_v1_e2_r3"])
def test_lookahead_with_moving_buffers(name, split_all):
    """The recipe of test_compact_seen_set_and_fixed_ring_match_golden: the seen set goes compact after
    2^10 slots and the ring is pinned at ~60 % of the live frontier's peak, so buffers move mid-level,
    the ring wraps and commits reuse the space of chunks already expanded -- under look-ahead."""
    split_all.setenv("RMC_LOOKAHEAD", "1")
    g = LEVELS[name]
    probe, res0 = run_cfg(g, **KW)
    peak = res0.frontier_peak_bytes
    probe.close()
    slots = 1 << max(12, (int(g["distinct"] / 0.6)).bit_length())
    ring = int(0.6 * peak) + 4 * CHUNK * 36 + 4096
    mc, res = run_cfg(g, compact_log2=10, seen_log2=8, seen_mem_bytes=8 * slots, frontier_mem_bytes=ring, **KW)
    check_levels(g, res)
    assert res.seen_slot_bytes == 8 and res.seen_slots == slots
    assert res.frontier_ring_bytes <= max(ring, 4 * CHUNK * 36 * 2)
    if name in TRACES:
        assert trace_of(mc) == golden_trace(TRACES[name])
    mc.close()


def test_lookahead_with_event_timing(split_all):
    """Timing as bench.py sets it (the expansion's phase only): the run completes, every chunk's
    expansion is counted once -- a look-ahead one after its own stream's events -- and took time."""
    split_all.setenv("RMC_LOOKAHEAD", "1")
    g = LEVELS["n3_v2_e1_r3"]
    mc, res = run_cfg(g, timing_phases=1 << PH_HASH, **KW)
    check_levels(g, res)
    cp = chunk_parents(g)
    for ls in res.levels[1:]:
        assert ls.kernel_launches[PH_HASH] == -(-ls.expanded // cp), ls
        assert ls.kernel_ms[PH_HASH] > 0, ls
    mc.close()
