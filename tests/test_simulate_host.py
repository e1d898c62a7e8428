"""CPU tests of simulation mode's host side: the choice function (include/rmc.h rmc_simulate) and the
launcher's argument checks.  No compute call is made here."""
import subprocess

import pytest

import raftmc
from test_host import LAUNCHER

# (seed, walk, step) -> r, then the index among c = 1, 2, 7, 88, 306 successors
VECTORS = [
    ((0, 0, 0), 0xe220a839, (0, 1, 6, 77, 270)),
    ((1, 0, 0), 0x910a2dec, (0, 1, 3, 49, 173)),
    ((1, 69, 15), 0xbe10091b, (0, 1, 5, 65, 227)),
    ((0xDEADBEEF, 12345, 99), 0xac02dca6, (0, 1, 4, 59, 205)),
    ((2**64 - 1, 2**40 + 7, 4000), 0x638952e8, (0, 0, 2, 34, 118)),
]
COUNTS = (1, 2, 7, 88, 306)


@pytest.mark.parametrize("args,r,idx", VECTORS)
def test_sim_choice_check_vectors(args, r, idx):
    assert raftmc.sim_random(*args) == r
    assert tuple(raftmc.sim_choice(*args, c) for c in COUNTS) == idx


def test_sim_choice_is_in_range():
    for c in (1, 3, 64, 306):
        for step in range(50):
            assert 0 <= raftmc.sim_choice(7, 11, step, c) < c


@pytest.mark.parametrize("extra", [
    ["-simulate", "-gpus", "2"],
    ["-simulate", "-recover", "states/x"],
    ["-simulate", "-checkpoint", "5"],
    ["-simulate", "-depth", "0"],
    ["-simulate", "num=abc"],
    ["-simulate", "num="],
    ["-simulate", "num=0"],
    ["-simulate", "num=12x"],
    ["-simulate", "file=trace"],
])
def test_launcher_rejects_simulate_combinations(extra):
    """Refused with TLC's exit code 150 from the argument check: no file is read and no device touched
    (the spec named here does not exist)."""
    r = subprocess.run([LAUNCHER] + extra + ["NoSuchSpec.tla"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 150, r.stdout + r.stderr
    assert "usage: raftmc" in r.stderr and "-simulate" in r.stderr
    assert r.stdout == ""


def test_launcher_usage_names_the_simulation_flags():
    r = subprocess.run([LAUNCHER, "-bogus", "Raft.tla"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 150
    for word in ("-simulate", "num=N", "-depth", "-seed", "unbounded"):
        assert word in r.stderr
