#!/bin/bash
# Drop-in for kikimo/tla-raft's myrun.sh (myrun.sh:3): same flags, same inputs
# (Raft.tla, Raft.cfg in the current directory), TLC-style output teed to raft.log --
# the state space is explored on the MI355X by librmc instead of TLC.
# GPU-specific flags go through with the rest, next to -gpus N:
#   -canreach NAME | -canreach NAME=FALSE   (repeatable) after the verdict, how many distinct states can still reach
#   a state on which invariant NAME is TRUE (FALSE), and the behaviour to the first one that cannot
#   -eventually NAME[=FALSE] | -leadsto Q[=FALSE] P[=FALSE]   (repeatable) from how many states NAME must follow on every
#   fair behaviour, how many can avoid it forever, and a counter-example (a lasso or a dead end) when the property fails
#   -scc   the strongly connected components of the state graph
#   -fullstate   identify states by all twelve variables instead of the cfg's VIEW (which leaves out electionCount,
#   restartCount, pendingResponse and valSent); one extra line after the header, the counters are then of whole states
DIR=$(cd "$(dirname "$0")" && pwd)
"$DIR/build/raftmc" -deadlock -workers 4 -config Raft.cfg Raft.tla $@ 2>&1 | tee raft.log
