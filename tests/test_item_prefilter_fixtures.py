"""What the inputs of tests/test_gpu_item_prefilter.py make the split expansion's item pre-filter
(RMC_ITEM_PREFILTER, k_expand_items) do, recounted on the CPU with tools/item_outcomes.py over raft_ref: every
branch of the filter -- a dropped and a kept item of each class it decides, a self-loop, slots switched off with
and without a lookup, parents left with no item, with self-loops only and with nothing -- must be taken by the
fixtures, so a regenerated fixture cannot silently stop exercising one.  The counts cover both steps the filter was
built with: step A (bit 0, kept) and step B (bit 1: the reply's membership for ResponseVote / FollowerAccept /
RejectEntry, measured and dropped -- bit 1 is ignored now)."""
import gzip
import json
import os
import sys
from collections import Counter

import raft_ref as R
import raftmc
from conftest import GOLDEN

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import item_outcomes as IO  # noqa: E402

with gzip.open(os.path.join(GOLDEN, "roots.json.gz"), "rt") as _f:
    ROOTS = json.load(_f)


def count(cfg, states):
    """(outcomes summed, parents with no item left at RMC_ITEM_PREFILTER=3, with successors that are all
    self-loops, with no successor at all)"""
    tot, none, selfonly, nothing = Counter(), 0, 0, 0
    for st in states:
        k = IO.outcomes(cfg, st)
        tot.update(k)
        nsucc = sum(v for (c, o), v in k.items() if not o.startswith("off"))
        none += IO.survivors(k, 3) == 0
        selfonly += nsucc > 0 and nsucc == k["AE", "self"]
        nothing += nsucc == 0
    return tot, none, selfonly, nothing


def root_states(e):
    return [R.state_from_json(raftmc.unpacked_to_state(r, e["n"], e["V"])) for r in e["roots"]]


def cfg_of(e):
    return R.Config(n=e["n"], V=e["V"], max_election=e["E"], max_restart=e["R"], become_follower=e["bf"])


def test_n3_v2_roots_take_every_branch():
    e = ROOTS["n3_v2"]
    assert len(e["roots"]) == 251 and min(e["root_msgs"]) >= 45 and max(e["root_msgs"]) <= 64
    tot, none, selfonly, nothing = count(cfg_of(e), root_states(e))
    assert (tot["HAR", "off"], tot["HAR", "staged"]) == (180, 87)
    assert (tot["AE", "self"], tot["AE", "off"], tot["AE", "accepted"], tot["AE", "rejected"]) == (210, 153, 120, 480)
    assert (tot["RV", "off"], tot["RV", "staged"]) == (1024, 77)
    assert (tot["BL", "off"], tot["BL", "staged"]) == (37, 39)
    assert (tot["LAE", "off_cheap"], tot["LAE", "off_member"]) == (135, 31) and tot["LAE", "staged"] > 0
    assert tot["CR", "off"] and tot["CR", "staged"] and tot["LCC", "off"] and tot["RS", "staged"] and tot["BC", "staged"]
    assert tot["UT", "staged"] and tot["UT2", "staged"]
    assert (none, selfonly, nothing) == (6, 3, 3)


def test_five_server_roots_take_the_wide_kernels_branches():
    """n5_v1 and its BecomeFollower twin: LeaderCanCommit on and off, every message class dropped and kept; with
    BecomeFollower the second candidate exists (outcomes asserts it belongs to UT / UT2 items only)."""
    for name in ("n5_v1", "bf_n5_v1"):
        e = ROOTS[name]
        assert e["lanes"] == 128
        tot, _, _, _ = count(cfg_of(e), root_states(e))
        for kind in (("LCC", "off"), ("LCC", "staged"), ("HAR", "off"), ("HAR", "staged"), ("RV", "off"), ("RV", "staged"),
                     ("AE", "self"), ("AE", "off"), ("AE", "accepted"), ("AE", "rejected"), ("BL", "off"), ("BL", "staged"),
                     ("LAE", "off_cheap"), ("LAE", "off_member"), ("LAE", "staged"), ("CR", "off"), ("CR", "staged"),
                     ("UT", "staged"), ("UT2", "staged")):
            assert tot[kind] > 0, (name, kind)
    cfg = cfg_of(ROOTS["bf_n5_v1"])
    assert any(a == R.A_BF for st in root_states(ROOTS["bf_n5_v1"])[:20] for (_, a, _), _ in R.successors(cfg, st))


def test_exhaustive_runs_have_parents_without_items():
    r = R.bfs(R.Config(n=3, V=2, max_election=1, max_restart=3), keep_states=True)
    assert r.distinct == 10501
    _, none, selfonly, nothing = count(R.Config(n=3, V=2, max_election=1, max_restart=3), r.states)
    assert (none, selfonly, nothing) == (2253, 2248, 5)
    cfg = R.Config(n=2, V=1, max_election=2, max_restart=0)
    r = R.bfs(cfg, keep_states=True)
    assert r.distinct == 327
    tot, none, selfonly, nothing = count(cfg, r.states)
    assert nothing == 10 and none >= nothing and selfonly > 0
    # step A alone (RMC_ITEM_PREFILTER = 1) leaves a parent of this run without any item
    assert sum(IO.survivors(IO.outcomes(cfg, st), 1) == 0 for st in r.states) >= 1
    for c in IO.MSG_CLASSES + IO.SLOT_CLASSES:
        # (MaxRestart = 0: Restart is never in a leader's range; two servers: no candidate beside a leader of its term)
        if c not in ("RS", "UT2"):
            assert sum(v for (cc, _), v in tot.items() if cc == c) > 0, c
    # (two servers: every AppendReq at a follower in its term matches its log -- none rejected, none disabled)
    for kind in (("HAR", "off"), ("HAR", "staged"), ("RV", "off"), ("RV", "staged"), ("AE", "self"),
                 ("AE", "accepted"), ("BL", "off"), ("BL", "staged"), ("LAE", "off_cheap"), ("LAE", "off_member"),
                 ("LCC", "off"), ("LCC", "staged"), ("CR", "off"), ("CR", "staged")):
        assert tot[kind] > 0, kind
