"""Seeded-search fixtures (tests/golden/roots.json.gz, rmc_init_from) without a device: the fixture is
self-consistent, the generator reproduces its small entries, the conditions that make the entries worth running
hold (they are conditions, not measurements), raft_ref.py rechecks one first expansion, and the library
exports the hook within ABI 5."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

import raft_ref as R
import raftmc
from conftest import GOLDEN, ROOT

sys.path.insert(0, GOLDEN)
import make_golden_roots as M  # noqa: E402

with gzip.open(os.path.join(GOLDEN, "roots.json.gz"), "rt") as _f:
    ROOTS = json.load(_f)
COUNTING = ["n5_v1", "n4_v1", "n5_v2", "bf_n5_v1", "n3_v2"]
ERRORS = ["cap_n5_v1", "cap_n3_v2", "assert_n5_v1", "invroot_n3_v2"]
LEVEL_KEYS = ("expanded", "generated", "new_states", "self_loops")


def test_entries_and_size():
    assert list(ROOTS) == COUNTING + ERRORS == list(M.ENTRIES)
    assert os.path.getsize(os.path.join(GOLDEN, "roots.json.gz")) < os.path.getsize(os.path.join(GOLDEN, "successors.json"))
    for name, e in ROOTS.items():
        spec = M.ENTRIES[name]
        assert (e["n"], e["V"], e["E"], e["R"], e["bf"], e["lanes"], e["kind"]) == \
               (spec["n"], spec["V"], 3, 3, spec["bf"], spec["lanes"], spec["kind"])
        assert len(e["roots"]) == e["n_given"] == spec["roots"]
        for r in e["roots"]:  # a row is exactly as long as its message count says
            assert len(r) == raftmc.unpacked_len(e["n"], e["V"], r[raftmc.unpacked_len(e["n"], e["V"], 0) - 1])
    assert ROOTS["bf_n5_v1"]["bf"] and ROOTS["n5_v2"]["V"] == 2  # more than 256 slots; the largest successor stride


@pytest.mark.parametrize("name", COUNTING)
def test_counting_entry_is_consistent_and_meets_the_conditions(name):
    e = ROOTS[name]
    n, m, lanes = e["n_given"], e["m"], e["lanes"]
    assert 200 <= n <= 260 and n > 64 and n % 16 != 0 and m == n and e["stop"] is None
    l1, l2 = e["levels"]
    assert (l1["level"], l2["level"]) == (1, 2)
    assert l1["expanded"] == m and l2["expanded"] == l1["new_states"] == l1["queue"] and l2["queue"] == l2["new_states"]
    assert l1["total_generated"] == n + l1["generated"] and l2["total_generated"] == l1["total_generated"] + l2["generated"]
    assert l1["total_distinct"] == m + l1["new_states"] and l2["total_distinct"] == l1["total_distinct"] + l2["new_states"]
    assert e["states"] == l2["total_distinct"] and e["edges"] == l1["generated"] + l2["generated"]
    assert e["edges_per_level"] == [l1["generated"], e["edges"]]
    assert max(l1["new_states"], l2["new_states"]) <= 300_000
    # the states the suite's searches do not reach
    msgs = e["root_msgs"]
    assert len(msgs) == m and max(e["max_msgs"]) <= lanes and e["max_msgs"][1:] == [l1["max_msgs"], l2["max_msgs"]]
    if lanes == 128:
        assert 2 * sum(1 for x in msgs if x > 64) >= m
        assert sum(1 for x in msgs if x >= 120) >= 10
        assert e["max_msgs"][2] >= 126
    else:
        assert all(45 <= x <= 64 for x in msgs) and 2 * sum(1 for x in msgs if x > 44) >= m
        assert max(e["max_msgs"]) == 64
    assert l1["self_loops"] > 0 and l2["self_loops"] > 0
    # coverage: every action of Next fires, but for the ones the fixture names
    cov = e["coverage"]
    for a, act in enumerate(raftmc.ACTIONS):
        if act in cov["cannot_fire"]:
            assert cov["generated"][a] == cov["distinct"][a] == 0 and cov["cannot_fire"][act]
        else:
            assert cov["generated"][a] > 0, act
    assert set(cov["cannot_fire"]) == ({"FollowerAppendEntry"} if e["bf"] else {"FollowerAppendEntry", "BecomeFollower"})
    assert n + sum(cov["generated"]) == l2["total_generated"] and m + sum(cov["distinct"]) == e["states"]
    # continuation: Inv (first in bit order) holds everywhere; a state is attributed to one invariant at most
    cont = e["continuation"]
    assert list(cont) == list(raftmc.INVARIANT_BY_BIT) and cont["Inv"] == [0, 0, 0]
    for lvl, size in enumerate([m, l1["new_states"], l2["new_states"]]):
        assert sum(cont[nm][lvl] for nm in cont) <= size
    assert sum(sum(v) for v in cont.values()) > 0


def test_error_entries():
    for name in ("cap_n5_v1", "cap_n3_v2"):
        e = ROOTS[name]
        assert e["stop"]["status"] == "capacity" and e["stop"]["level"] == 2 and len(e["levels"]) == 1
        assert e["levels"][0]["max_msgs"] <= e["lanes"] and e["m"] == e["n_given"]
        lo = e["m"]
        assert lo <= e["stop"]["parent_gid"] < lo + e["levels"][0]["new_states"]  # a state of level 2
    e = ROOTS["assert_n5_v1"]
    s = e["stop"]
    assert s["status"] == "assert" and s["level"] == 1 and 0 < s["parent_gid"] < e["m"] - 1
    assert s["queue"] == e["m"] - s["parent_gid"] - 1 + s["level_new"] and s["distinct"] == e["m"] + s["level_new"]
    assert s["generated"] == e["n_given"] + s["level_generated"]
    e = ROOTS["invroot_n3_v2"]
    s = e["stop"]
    assert e["n_given"] == e["m"] + 1 and s["status"] == "violation" and s["invariant"] == "Inv"
    assert 0 < s["root_gid"] < e["m"] and (s["generated"], s["distinct"], s["queue"], s["depth"]) == (e["n_given"], e["m"], 0, 1)


@pytest.mark.parametrize("name", ["cap_n3_v2", "invroot_n3_v2", "assert_n5_v1"])
def test_generator_reproduces_the_entry(name):
    got = json.loads(json.dumps(M.one_entry(name)[1]))
    assert got == ROOTS[name]


def test_raft_ref_rechecks_the_first_expansion_of_n3_v2():
    """raft_ref.py alone (its successors, its exact canonical classes) on the 251 roots: the first expansion's
    counts, and the duplicate-class root of invroot_n3_v2 is one class by R.canonical as well."""
    e = ROOTS["n3_v2"]
    cfg = M.ref_cfg(M.ENTRIES["n3_v2"])
    got = M.ref_first_expansion(cfg, e["roots"], e["n"], e["V"])
    assert got == {k: e["levels"][0][k] for k in LEVEL_KEYS} == e["ref_first_expansion"]
    e = ROOTS["invroot_n3_v2"]
    classes = [R.canonical(cfg, R.state_from_json(raftmc.unpacked_to_state(r, e["n"], e["V"]))) for r in e["roots"]]
    assert len(set(classes)) == e["m"] and classes[7] == classes[3] and e["roots"][7] != e["roots"][3]
    kept = list(dict.fromkeys(classes))
    bad_row = e["roots"][classes.index(kept[e["stop"]["root_gid"]])]
    assert R.INV_FUNCS["Inv"](cfg, R.state_from_json(raftmc.unpacked_to_state(bad_row, e["n"], e["V"]))) is False
    for g in range(e["stop"]["root_gid"]):  # every kept root before it is clean
        row = e["roots"][classes.index(kept[g])]
        assert R.INV_FUNCS["Inv"](cfg, R.state_from_json(raftmc.unpacked_to_state(row, e["n"], e["V"]))) is True


def test_library_exports_init_from_within_abi_5():
    lib = raftmc.load_library()
    assert hasattr(lib, "rmc_init_from") and lib.rmc_abi_version() == 5
    with open(os.path.join(ROOT, "include", "rmc.h")) as f:
        header = f.read()
    assert "#define RMC_ABI_VERSION 5" in header and "int rmc_init_from(void *ctx, const int32_t *unpacked" in header
    assert hasattr(raftmc.ModelChecker, "init_from")
