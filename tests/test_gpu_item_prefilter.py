"""The split expansion's item pre-filter (RMC_ITEM_PREFILTER, rmc_kernels.hip k_expand_items): bit 0 keeps
an AppendResp whose HandleAppendResp guard fails, and every slot whose guards fail without a lookup, from
becoming items.  Bit 1 was the same for the VoteReqs / AppendReqs at a follower whose reply is in msgs already;
it was measured and dropped and is ignored, so 3 runs what 1 runs.  The settings 0 (every
item listed), 1 and 3 must give the same search, exactly: every comparison is against the goldens (tests/golden/,
from oracle/) or raft_ref.bfs run here.

What each input makes the filter do is recounted on the CPU by tests/test_item_prefilter_fixtures.py: the 251
n3_v2 roots of 45-64 messages take every branch (dropped and kept items of each class, counted self-loops,
slots off by the cheap guards and by membership, roots with self-loops only and with nothing); n2_v1_e2_r0 has
ten parents with no successor at all, one of them left without any item by bit 0 alone."""
import json
import os

import pytest

import raft_ref as R
import raftmc
from conftest import GOLDEN
from test_gpu import (LEVELS, LEVELS_BF, LEVELS_ERR, TRACES, TRACES_ERR, check_levels, run_cfg)
from test_gpu_roots import ROOTS, check_counting

pytestmark = pytest.mark.gpu

with open(os.path.join(GOLDEN, "levels_highterm.json")) as _f:
    LEVELS_HIGH = json.load(_f)

SETTINGS = ("0", "1", "3")


def level_counts(res):
    return [(ls.expanded, ls.generated, ls.new_states, ls.self_loops, ls.new_bytes) for ls in res.levels]


def trace_of(mc):
    return [(list(k) if k else None, st) for k, st in mc.trace()]


def golden_trace(t):
    return [(e["key"], e["state"]) for e in t["steps"]]


# ---- the roots: two levels from states of many messages, on every path the expansion takes ------------------
# (tests/test_gpu_roots.py PATHS: split chunks whole; cut into 64-parent chunks with the look-ahead on and off; a
# sharded split round, where self-loops stay items; the plain device loop, whose fused kernel lists as with 0)
ROOT_PATHS = ["split_lookahead", "chunks_split", "chunks_split_nolookahead", "virtual2_split", "device_loop"]


def roots_on(name, path, pf, monkeypatch):
    monkeypatch.setenv("RMC_ITEM_PREFILTER", pf)
    if path == "chunks_split_nolookahead":
        monkeypatch.setenv("RMC_LOOKAHEAD", "0")
        path = "chunks_split"
    check_counting(ROOTS[name], path, monkeypatch)


@pytest.mark.parametrize("pf", SETTINGS)
@pytest.mark.parametrize("path", ROOT_PATHS)
def test_n3_v2_roots(path, pf, monkeypatch):
    roots_on("n3_v2", path, pf, monkeypatch)


@pytest.mark.parametrize("pf", SETTINGS)
@pytest.mark.parametrize("grid", ["1", "3"])
def test_n3_v2_roots_blocks_take_several_batches(grid, pf, monkeypatch):
    """251 roots are four batches: one block walks them all, three take 2, 1 and 1 -- the per-batch state the
    filter adds (the slot masks, the counted self-loops) starts afresh in each."""
    monkeypatch.setenv("RMC_ITEMS_GRID", grid)
    roots_on("n3_v2", "split_lookahead", pf, monkeypatch)


@pytest.mark.parametrize("pf", SETTINGS)
@pytest.mark.parametrize("path", ["split_lookahead", "chunks_split"])
@pytest.mark.parametrize("name", ["n5_v1", "bf_n5_v1"])
def test_five_server_roots(name, path, pf, monkeypatch):
    """The msg_cap-128 kernels (a five-server slot mask fills 60 bits of its word), LeaderCanCommit on and off,
    and with BecomeFollower the message items' second candidate, which no filtered class has."""
    roots_on(name, path, pf, monkeypatch)


# ---- exhaustive small runs on the split path -------------------------------------------------------------------
def across_settings(g, monkeypatch, trace=None, **kw):
    monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    counts = []
    for pf in SETTINGS:
        monkeypatch.setenv("RMC_ITEM_PREFILTER", pf)
        mc, res = run_cfg(g, device_levels=1, **kw)
        check_levels(g, res)
        if trace is not None:
            assert trace_of(mc) == golden_trace(trace)
        counts.append(level_counts(res))
        mc.close()
    assert counts[0] == counts[1] == counts[2]  # (self-loops per level among them)
    return counts[0]


@pytest.mark.parametrize("name,levels", [("n3_v2_e1_r3", LEVELS), ("n2_v1_e2_r0", LEVELS_HIGH),
                                         ("bf_n3_v2_e1_r3", LEVELS_BF)])
def test_exhaustive_runs(name, levels, monkeypatch):
    counts = across_settings(levels[name], monkeypatch)
    assert sum(c[3] for c in counts) > 0  # self-loops were counted


@pytest.mark.parametrize("name", ["seeded_n3_v2_e2_r3"])
def test_seeded_median(name, monkeypatch):
    """RaftSeeded: LeaderCanCommit's median over all servers (the mask's threshold is P.seeded's)."""
    across_settings(LEVELS[name], monkeypatch, trace=TRACES[name])


@pytest.mark.parametrize("name", ["sb_n3_v2_e2_r3", "cpl_n3_v2_e1_r3"])
def test_quirk_variants_end_in_their_errors(name, monkeypatch):
    """RaftSplitBrain (BecomeLeader's quorum 1 in the mask; ends in UpdateTerm's Assert, an IC_UT2 item the
    filter never touches) and RaftCommitPastLog (no Min in the new commitIndex, which decides whether an
    accepted entry is the parent itself; ends in Inv's evaluation error)."""
    across_settings(LEVELS_ERR[name], monkeypatch, trace=TRACES_ERR[name])


# ---- deadlock: a parent with only self-loops is none, a parent with nothing is ---------------------------------
def test_deadlock_golden(monkeypatch):
    name = "deadlock_n3_v1_e1_r3"
    across_settings(LEVELS[name], monkeypatch, trace=TRACES[name])


def test_deadlock_against_raft_ref(monkeypatch):
    """n2_v1_e2_r0 with -deadlock: the first of its ten parents without a successor stops the run, with TLC's
    counters at the report; the parents whose successors are all self-loops before it do not."""
    exp = R.bfs(R.Config(n=2, V=1, max_election=2, max_restart=0, check_deadlock=True))
    assert exp.verdict == "deadlock"
    monkeypatch.setenv("RMC_SPLIT_MIN", "1")
    for pf in SETTINGS:
        monkeypatch.setenv("RMC_ITEM_PREFILTER", pf)
        with raftmc.ModelChecker(raftmc.ModelConfig(n_servers=2, n_vals=1, max_election=2, max_restart=0,
                                                    check_deadlock=True, device_levels=1)) as mc:
            res = mc.run()
            assert (res.status, res.generated, res.distinct, res.queue, res.trace_len) == \
                   ("deadlock", exp.generated, exp.distinct, exp.queue_left, len(exp.trace))
            assert [st for _, st in mc.trace()] == [R.state_to_json(st) for _, st in exp.trace]
