#!/usr/bin/env python3
"""What becomes of the items the split expansion (k_expand_items) lists for a parent, counted on the CPU.

A parent's items are every message some action may receive, by its class alone (msg_class: the message's
term and type against its destination's term and role), and every non-message slot its servers' roles
allow (slot_range).  Each item's outcome is read off raft_ref.successors: it stages a successor, it is the
parent itself (a FollowerAcceptEntry that changes nothing: counted, never staged), or it is disabled.  The
item pre-filter (RMC_ITEM_PREFILTER, step A) drops the disabled ones it can decide without a lookup; step B
(bit 1: the reply's membership for ResponseVote / FollowerAccept / RejectEntry, measured and dropped, DESIGN.md
section 4) would have dropped the rest.  This is the count of how many items each setting leaves.

As a script: the reachable Raft.cfg walk states of tests/golden/successors_deep.json.gz, per class
listed / staged / self-loop / disabled per parent (profiles/item_outcomes.txt).  As a module:
outcomes(cfg, st) and survivors(kinds, prefilter), used by tests/test_item_prefilter_fixtures.py.

usage: python tools/item_outcomes.py [--entry raftcfg_n3_v2_e3_r3]"""
import argparse
import gzip
import json
import os
import sys
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import raft_ref as R  # noqa: E402

MSG_CLASSES = ("UT", "UT2", "RV", "AE", "HAR")
SLOT_CLASSES = ("BC", "BL", "CR", "LAE", "LCC", "RS")


def msg_class(st, m):
    """The kernel's msg_class: None for a message no action can receive."""
    s, mt, typ = R.mdst(m), R.mterm(m), R.mtype(m)
    ct, role = st.currentTerm[s], st.role[s]
    if mt > ct:
        return "UT"
    if mt < ct:
        return None
    if typ == "AppendReq":
        return "UT2" if role != R.FOLLOWER else "AE"
    if typ == "VoteReq":
        return "RV" if role == R.FOLLOWER else None
    if typ == "AppendResp":
        return "HAR" if role == R.LEADER else None
    return None


def slot_items(cfg, st, s):
    """The kernel's slot_range: (class, witness) of the slots server s's role allows."""
    role = st.role[s]
    if role == R.LEADER:
        out = [("CR", v) for v in range(cfg.V)] + [("LAE", d) for d in range(cfg.n) if d != s] + [("LCC", 0)]
        return out + ([("RS", 0)] if st.restartCount < cfg.max_restart else [])
    out = [("BC", 0)] if st.electionCount < cfg.max_election else []
    return out + ([("BL", 0)] if role == R.CANDIDATE else [])


ACTION_OF = {"BC": R.A_BC, "BL": R.A_BL, "CR": R.A_CR, "LAE": R.A_LAE, "LCC": R.A_LCC, "RS": R.A_RS}


def outcomes(cfg, st):
    """Counter of (class, outcome) over the items listed for st.  Outcomes: "staged", "self", "off"; for AE
    "accepted" / "rejected" instead of "staged"; for LAE "off_cheap" (nextIndex or pendingResponse) and
    "off_member" (the AppendReq is in msgs) instead of "off".  A BecomeFollower successor of the variant
    counts with its message's item (classes UT and UT2 only: asserted)."""
    succ = R.successors(cfg, st)
    by_key = {}
    for (s, a, w), t in succ:
        by_key.setdefault((s, a, w), t)
    msgs = sorted(st.msgs)
    kinds = Counter()
    for w, m in enumerate(msgs):
        c = msg_class(st, m)
        s = R.mdst(m)
        got = {a: by_key.get((s, a, w)) for a in (R.A_UT, R.A_BF, R.A_RV, R.A_FAE, R.A_FRE, R.A_HAR)}
        if c is None or c in ("RV", "AE", "HAR"):
            assert got[R.A_UT] is None and got[R.A_BF] is None  # no BecomeFollower candidate, no UpdateTerm
        if c is None:
            assert all(v is None for v in got.values())
            continue
        if c == "AE":
            if got[R.A_FAE] is not None:
                kinds[c, "self" if got[R.A_FAE] == st else "accepted"] += 1
            else:
                kinds[c, "rejected" if got[R.A_FRE] is not None else "off"] += 1
        else:
            a = {"UT": R.A_UT, "UT2": R.A_UT, "RV": R.A_RV, "HAR": R.A_HAR}[c]
            kinds[c, "staged" if got[a] is not None else "off"] += 1
            if got[a] is not None:
                assert got[a] != st
    for s in range(cfg.n):
        for c, w in slot_items(cfg, st, s):
            t = by_key.get((s, ACTION_OF[c], w))
            if t is not None:
                assert t != st
                kinds[c, "staged"] += 1
            elif c == "LAE":
                cheap = st.nextIndex[s][w] <= len(st.logs[s]) + 1 and not st.pendingResponse[s][w]
                kinds[c, "off_member" if cheap else "off_cheap"] += 1
            else:
                kinds[c, "off"] += 1
    # every successor belongs to a listed item
    assert sum(v for (c, o), v in kinds.items() if not o.startswith("off")) == \
        len([1 for (s, a, w), _ in succ if a != R.A_BF])
    return kinds


def survivors(kinds, prefilter, self_apart=True):
    """Items still listed under RMC_ITEM_PREFILTER = prefilter (self_apart: the launch sets self-loops apart)."""
    n = 0
    for (c, o), v in kinds.items():
        if (prefilter & 1) and ((c == "HAR" and o == "off") or (c in SLOT_CLASSES and o in ("off", "off_cheap"))):
            continue
        if (prefilter & 2) and c in ("RV", "AE") and (o == "off" or (o == "self" and self_apart)):
            continue
        n += v
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entry", default="raftcfg_n3_v2_e3_r3")
    a = ap.parse_args()
    with gzip.open(os.path.join(ROOT, "tests", "golden", "successors_deep.json.gz"), "rt") as f:
        g = json.load(f)[a.entry]
    cfg = R.Config(n=g["n"], V=g["V"], max_election=g["E"], max_restart=g["R"])
    tot, n, nmsg, nsucc, nself, surv = Counter(), 0, 0, 0, 0, [0, 0, 0]
    for it in g["items"]:
        if it["assert_fails"] or it.get("synthetic"):
            continue
        st = R.state_from_json(it["state"])
        k = outcomes(cfg, st)
        tot.update(k)
        n += 1
        nmsg += len(st.msgs)
        nsucc += sum(v for (c, o), v in k.items() if not o.startswith("off"))
        nself += k["AE", "self"]
        for i, pf in enumerate((0, 1, 3)):
            surv[i] += survivors(k, pf)
    print(f"{a.entry}: {n} states, {nmsg / n:.1f} messages, {nsucc / n:.2f} successors per state, "
          f"{100.0 * nself / nsucc:.1f} % self-loops")
    print(f"{'class':6s} {'listed':>8s} {'staged':>8s} {'self':>8s} {'disabled':>9s}   (per parent)")
    lt = st_ = sf = of = 0
    for c in MSG_CLASSES + SLOT_CLASSES:
        listed = sum(v for (cc, o), v in tot.items() if cc == c)
        self_ = tot[c, "self"]
        off = sum(v for (cc, o), v in tot.items() if cc == c and o.startswith("off"))
        staged = listed - self_ - off
        lt, st_, sf, of = lt + listed, st_ + staged, sf + self_, of + off
        extra = ""
        if c == "AE":
            extra = f"   accepted {tot[c, 'accepted'] / n:.2f}, rejected {tot[c, 'rejected'] / n:.2f}"
        if c == "LAE":
            extra = f"   off by nextIndex / pendingResponse {tot[c, 'off_cheap'] / n:.2f}, by m in msgs {tot[c, 'off_member'] / n:.2f}"
        print(f"{c:6s} {listed / n:8.2f} {staged / n:8.2f} {self_ / n:8.2f} {off / n:9.2f}{extra}")
    print(f"{'total':6s} {lt / n:8.2f} {st_ / n:8.2f} {sf / n:8.2f} {of / n:9.2f}")
    print("items per parent still listed: RMC_ITEM_PREFILTER=0 %.2f, =1 %.2f, =3 %.2f" % tuple(x / n for x in surv))
    print("per batch of 64 parents: %.0f, %.0f, %.0f items (a round takes up to 256, whole parents)" % tuple(64 * x / n for x in surv))


if __name__ == "__main__":
    main()
