// raftmc -- TLC-compatible command line over librmc (the drop-in for myrun.sh:3).
//
//   raftmc [-deadlock] [-workers N] [-config Raft.cfg] [-device D] [-gpus N] [-msgcap C] [-seenlog2 K] Raft.tla
//   raftmc -coverage MIN ... Raft.tla   (TLC's -coverage: the per-action distinct:generated report at the end)
//   raftmc -continue ... Raft.tla       (TLC's -continue: search past invariant violations, count them per invariant)
//   raftmc -dump FILE | -dump dot[,actionlabels] FILE ... Raft.tla   (TLC's -dump: the state graph, FILE.dump / FILE.dot)
//   raftmc -canreach NAME[=FALSE] ... Raft.tla   (GPU-specific: which states can still reach one where NAME holds)
//   raftmc -fullstate ... Raft.tla      (GPU-specific: states are identified by all twelve variables, not the VIEW)
//   raftmc -simulate [num=N] [-depth D] [-seed S] [-deadlock] [-config Raft.cfg] [-device D] [-msgcap C] Raft.tla
//
// Accepts the flags myrun.sh passes to TLC (myrun.sh:3), reads the same Raft.tla /
// Raft.cfg, and prints TLC's result lines (states generated, distinct states, depth,
// the counterexample) so that parsers of raft.log keep working.  -simulate is TLC's simulation mode:
// seeded random behaviours of at most -depth states instead of the breadth-first search (rmc_simulate).  GPU-specific lines
// are printed after TLC's block.  Exit codes follow TLC's (0 ok, 11 deadlock,
// 12 safety violation, 14 Assert, 75 evaluation error, 150/151 spec/config errors).
#include <fcntl.h>
#include <signal.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <chrono>
#include <functional>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <filesystem>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "rmc.h"
#include "rmc_cfg.h"

namespace {

// rmc_trace_step.action ids (Raft.tla's Next disjuncts; 11 never appears, 12 only in the tla:420 variant)
const char *kActionNames[13] = {"BecomeCandidate", "UpdateTerm", "ResponseVote", "BecomeLeader",
                                "ClientReq", "LeaderAppendEntry", "FollowerAcceptEntry", "FollowerRejectEntry",
                                "HandleAppendResp", "LeaderCanCommit", "Restart", "FollowerAppendEntry",
                                "BecomeFollower"};
const char *kInvNames[7] = {"Inv", "NoSplitVote", "RaftCanCommt", "FollowerCanCommit", "CommitAll", "NoAllCommit",
                            "ExistLeaderAndCandidate"};

std::string now_str() {
    char buf[64];
    std::time_t t = std::time(nullptr);
    std::strftime(buf, sizeof buf, "%Y-%m-%d %H:%M:%S", std::localtime(&t));
    return buf;
}

// TLC's metadir name: states/YY-MM-DD-HH-MM-SS
std::string stamp_str() {
    char buf[64];
    std::time_t t = std::time(nullptr);
    std::strftime(buf, sizeof buf, "%y-%m-%d-%H-%M-%S", std::localtime(&t));
    return buf;
}

bool read_file(const std::string &path, std::string *out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::stringstream ss;
    ss << f.rdbuf();
    *out = ss.str();
    return true;
}

// Source range of each action definition body in the spec text: TLC prints
// "<Name line L, col C to line L2, col C2 of module M>" for trace steps.
struct Loc {
    int l0 = 0, c0 = 0, l1 = 0, c1 = 0;
};

// BecomeFollower (tla:226) is a disjunction of three actions; TLC names a step by the one taken,
// which role[s] of the step's first state decides
const char *kBfNames[3] = {"FollowerUpdateTerm", "CandidateToFollower", "LeaderToFollower"};

std::vector<Loc> action_locations(const std::string &tla, const std::vector<std::string> &names) {
    std::vector<std::string> lines;
    std::stringstream ss(tla);
    std::string ln;
    while (std::getline(ss, ln)) {
        if (!ln.empty() && ln.back() == '\r') ln.pop_back();
        lines.push_back(ln);
    }
    std::vector<Loc> locs(names.size());
    for (size_t a = 0; a < names.size(); a++) {
        const std::string head = names[a] == "Init" ? std::string("Init ==") : names[a] + "(s) ==";
        for (size_t i = 0; i < lines.size(); i++) {
            if (lines[i].compare(0, head.size(), head) != 0) continue;
            // body starts at the first non-blank character after "=="
            size_t li = i, col = head.size();
            while (li < lines.size()) {
                while (col < lines[li].size() && isspace((unsigned char)lines[li][col])) col++;
                if (col < lines[li].size()) break;
                li++;
                col = 0;
            }
            Loc L;
            L.l0 = (int)li + 1;
            L.c0 = (int)col + 1;
            // body ends at the last token before the next column-1 line: blank lines, comment-only
            // lines (tla:173 "\* /\ Print(...)" after BecomeLeader's last conjunct) and a line's
            // trailing "\*" comment are not part of the expression
            auto code_end = [&](size_t k) -> long {  // last code column (0-based) of line k, -1 if none
                const std::string &s = lines[k];
                size_t cut = s.find("\\*");
                long e = (long)std::min(cut, s.size()) - 1;
                while (e >= 0 && isspace((unsigned char)s[e])) e--;
                return e;
            };
            size_t j = li + 1;
            while (j < lines.size() && (lines[j].empty() || isspace((unsigned char)lines[j][0]))) j++;
            size_t e = j - 1;
            while (e > li && code_end(e) < 0) e--;
            L.l1 = (int)e + 1;
            L.c1 = (int)code_end(e) + 1;
            locs[a] = L;
            break;
        }
    }
    return locs;
}

struct Printer {
    const rmc::ParsedModel &pm;
    int n, V;
    std::string sv(int i) const { return i < 0 ? "None" : pm.servers[i]; }
    std::string fn_servers(const std::vector<std::string> &vals) const {
        std::string s = "(";
        for (int i = 0; i < n; i++) s += (i ? " @@ " : "") + pm.servers[i] + " :> " + vals[i];
        return s + ")";
    }
    std::string entry(int t, int v) const {
        return "[term |-> " + std::to_string(t) + ", val |-> " + (v < 0 ? std::string("None") : pm.vals[v]) + "]";
    }
    std::string state(const int32_t *u) const {
        int k = 0;
        std::vector<std::string> vf, ct, role, ci, logs;
        for (int i = 0; i < n; i++) vf.push_back(sv(u[k++]));
        for (int i = 0; i < n; i++) ct.push_back(std::to_string(u[k++]));
        static const char *rn[3] = {"Follower", "Candidate", "Leader"};
        for (int i = 0; i < n; i++) role.push_back(rn[u[k++]]);
        for (int i = 0; i < n; i++) ci.push_back(std::to_string(u[k++]));
        std::vector<int> ll;
        for (int i = 0; i < n; i++) ll.push_back(u[k++]);
        for (int i = 0; i < n; i++) {
            std::string s = "<<";
            for (int x = 1; x <= V + 1; x++) {
                int t = u[k], v = u[k + 1];
                k += 2;
                if (x <= ll[i]) s += (x > 1 ? ", " : "") + entry(t, v);
            }
            logs.push_back(s + ">>");
        }
        auto matrix = [&](bool boolean) {
            std::vector<std::string> rows;
            for (int i = 0; i < n; i++) {
                std::vector<std::string> r;
                for (int j = 0; j < n; j++) {
                    int v = u[k++];
                    r.push_back(boolean ? (v ? "TRUE" : "FALSE") : std::to_string(v));
                }
                rows.push_back(fn_servers(r));
            }
            return fn_servers(rows);
        };
        std::string mi = matrix(false), ni = matrix(false), pend = matrix(true);
        int ec = u[k++], rc = u[k++];
        std::string vs = "(";
        for (int v = 0; v < V; v++) vs += (v ? " @@ " : "") + pm.vals[v] + " :> " + (u[k++] < 0 ? "None" : "FALSE");
        vs += ")";
        if (V == 0) vs = "<<>>";
        int nm = u[k++];
        std::string msgs = "{";
        static const char *tn[4] = {"VoteReq", "VoteResp", "AppendReq", "AppendResp"};
        for (int q = 0; q < nm; q++, k += 8) {
            const int32_t *m = u + k;
            std::string r;
            switch (m[0]) {
            case 0:
                r = "[dst |-> " + sv(m[2]) + ", lastLogIndex |-> " + std::to_string(m[4]) + ", lastLogTerm |-> " +
                    std::to_string(m[5]) + ", src |-> " + sv(m[1]) + ", term |-> " + std::to_string(m[3]) +
                    ", type |-> VoteReq]";
                break;
            case 1:
                r = "[dst |-> " + sv(m[2]) + ", src |-> " + sv(m[1]) + ", term |-> " + std::to_string(m[3]) +
                    ", type |-> VoteResp]";
                break;
            case 2:
                r = "[dst |-> " + sv(m[2]) + ", entries |-> <<" + (m[7] < 0 ? "" : entry(m[7] / 8, m[7] % 8)) +
                    ">>, leaderCommit |-> " + std::to_string(m[6]) + ", prevLogIndex |-> " + std::to_string(m[4]) +
                    ", prevLogTerm |-> " + std::to_string(m[5]) + ", src |-> " + sv(m[1]) + ", term |-> " +
                    std::to_string(m[3]) + ", type |-> AppendReq]";
                break;
            default:
                r = "[dst |-> " + sv(m[2]) + ", prevLogIndex |-> " + std::to_string(m[4]) + ", src |-> " + sv(m[1]) +
                    ", succ |-> " + (m[5] ? "TRUE" : "FALSE") + ", term |-> " + std::to_string(m[3]) +
                    ", type |-> AppendResp]";
            }
            (void)tn;
            msgs += (q ? ",\n   " : "") + r;
        }
        msgs += "}";
        std::string o;
        o += "/\\ votedFor = " + fn_servers(vf) + "\n";
        o += "/\\ currentTerm = " + fn_servers(ct) + "\n";
        o += "/\\ logs = " + fn_servers(logs) + "\n";
        o += "/\\ matchIndex = " + mi + "\n";
        o += "/\\ nextIndex = " + ni + "\n";
        o += "/\\ commitIndex = " + fn_servers(ci) + "\n";
        o += "/\\ msgs = " + msgs + "\n";
        o += "/\\ role = " + fn_servers(role) + "\n";
        o += "/\\ electionCount = " + std::to_string(ec) + "\n";
        o += "/\\ restartCount = " + std::to_string(rc) + "\n";
        o += "/\\ pendingResponse = " + pend + "\n";
        o += "/\\ valSent = " + vs + "\n";
        return o;
    }
};

// -dump FILE / -dump dot[,actionlabels] FILE: the sink of rmc_set_graph.  States and edges arrive level by level;
// the dump file takes the states as they come, the dot file its node lines, while the edge lines wait in a
// temporary file and follow the last node (finish).  Both streams are buffered; a failed write makes the callback
// return non-zero, which fails the step (RMC_E_SINK).
struct DumpSink {
    std::string path, err;
    bool dot = false, labels = false;
    FILE *f = nullptr, *ef = nullptr;  // the file; dot: the edge lines so far
    const Printer *pr = nullptr;
    bool fail(const char *what) {
        if (err.empty()) err = std::string(what) + " " + path + ": " + std::strerror(errno);
        return false;
    }
    bool open() {
        f = std::fopen(path.c_str(), "w");
        if (!f) return fail("cannot open");
        if (!dot) return true;
        ef = std::tmpfile();
        if (!ef) return fail("cannot create the temporary edge file of");
        if (std::fputs("strict digraph DiskGraph {\nnodesep=0.35;\nsubgraph cluster_graph {\ncolor=\"white\";\n", f) < 0)
            return fail("cannot write");
        return true;
    }
    static std::string escape(const std::string &s) {  // a state as a dot label: no trailing newline
        std::string o;
        const size_t n = !s.empty() && s.back() == '\n' ? s.size() - 1 : s.size();
        for (size_t i = 0; i < n; i++) {
            if (s[i] == '\n') o += "\\n";
            else if (s[i] == '"') o += "\\\"";
            else if (s[i] == '\\') o += "\\\\";
            else o += s[i];
        }
        return o;
    }
    static int32_t on_states(void *user, uint64_t gid0, uint64_t n, const int32_t *u, size_t stride) {
        DumpSink *d = static_cast<DumpSink *>(user);
        for (uint64_t i = 0; i < n; i++) {
            const std::string st = d->pr->state(u + i * stride);
            const unsigned long long num = (unsigned long long)(gid0 + i + 1);
            const int rc = d->dot ? std::fprintf(d->f, "%llu [label=\"%s\"%s]\n", num, escape(st).c_str(),
                                                 gid0 + i == 0 ? ",style = filled" : "")
                                  : std::fprintf(d->f, "State %llu:\n%s\n", num, st.c_str());
            if (rc < 0) return d->fail("cannot write") ? 0 : 1;
        }
        return 0;
    }
    static int32_t on_edges(void *user, uint64_t n, const uint64_t *src, const uint32_t *key, const uint64_t *dst) {
        DumpSink *d = static_cast<DumpSink *>(user);
        if (!d->dot) return 0;
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t a = (key[i] >> 16) & 0xFFu;
            if (std::fprintf(d->ef, "%llu -> %llu [label=\"%s\",color=\"black\",fontcolor=\"black\"];\n",
                             (unsigned long long)(src[i] + 1), (unsigned long long)(dst[i] + 1),
                             d->labels && a < 13 ? kActionNames[a] : "") < 0)
                return d->fail("cannot write the temporary edge file of") ? 0 : 1;
        }
        return 0;
    }
    // the edge lines behind the nodes, the closing braces, and the file closed
    bool finish() {
        if (!f) return err.empty();
        if (dot) {
            char buf[1 << 16];
            if (std::fflush(ef) != 0 || std::fseek(ef, 0, SEEK_SET) != 0) return fail("cannot read back the edges of");
            for (size_t k; (k = std::fread(buf, 1, sizeof buf, ef)) > 0;)
                if (std::fwrite(buf, 1, k, f) != k) return fail("cannot write");
            if (std::ferror(ef)) return fail("cannot read back the edges of");
            if (std::fputs("}\n}\n", f) < 0) return fail("cannot write");
            std::fclose(ef);
            ef = nullptr;
        }
        FILE *g = f;
        f = nullptr;
        if (std::fclose(g) != 0) return fail("cannot write");
        return true;
    }
};

int usage(const char *msg) {
    std::fprintf(stderr, "raftmc: %s\nusage: raftmc [-deadlock] [-workers N] [-config FILE.cfg] [-device D] "
                         "[-gpus N [-onerank] [-shardmin K]] [-msgcap C] [-seenlog2 K] [-checkpoint MIN] [-metadir DIR] "
                         "[-recover DIR] [-coverage MIN] [-continue] [-dump [dot[,actionlabels]] FILE] [-canreach NAME[=FALSE]]... "
                         "[-fullstate] [-eventually NAME[=FALSE]]... [-leadsto Q[=FALSE] P[=FALSE]]... [-scc] FILE.tla\n"
                         "       raftmc -simulate [num=N] [-depth D] [-seed S] [-deadlock] [-config FILE.cfg] [-device D] "
                         "[-msgcap C] FILE.tla\n"
                         "  -coverage MIN  per-action coverage (distinct:generated) at the end of the search; the interval "
                         "is parsed as TLC's, only the final report is printed\n"
                         "  -continue  search past invariant violations: per violated invariant the first behaviour and the "
                         "number of violating states (TLC prints every one); exit code 12 if any\n"
                         "  -dump FILE  every distinct state in discovery order to FILE.dump; -dump dot FILE: the state graph "
                         "(states and every edge) to FILE.dot, with dot,actionlabels the edges carry their action's name; "
                         "one GPU, not with -simulate or -recover\n"
                         "  -canreach NAME[=FALSE]  (GPU-specific, repeatable) after the search: how many distinct states can "
                         "still reach a state on which invariant NAME is TRUE (=FALSE: is FALSE), and the behaviour to the first "
                         "that cannot; NAME is one of Inv NoSplitVote RaftCanCommt FollowerCanCommit CommitAll NoAllCommit "
                         "ExistLeaderAndCandidate, in the cfg or not; one GPU, not with -simulate or -recover\n"
                         "  -fullstate  (GPU-specific) identify states by all twelve variables instead of the cfg's VIEW, which "
                         "leaves out electionCount, restartCount, pendingResponse and valSent; combines with every option "
                         "of the search, not with -simulate (which keeps no set of states)\n"
                         "  -eventually NAME[=FALSE]  (GPU-specific, repeatable) after the search: from how many distinct states "
                         "every fair behaviour (a maximal path of the state graph) must reach a state on which NAME is TRUE "
                         "(=FALSE: is FALSE), how many can avoid it forever, and a counter-example if Init can; the fairness "
                         "is assumed, not the spec's: the exit code stays the search's\n"
                         "  -leadsto Q[=FALSE] P[=FALSE]  (likewise) Q ~> P: a counter-example if a state where Q holds can avoid P\n"
                         "  -scc  (likewise) the strongly connected components of the state graph, self-loops ignored\n"
                         "  -simulate  random behaviours instead of the breadth-first search; num=N of them (default "
                         "1000000; TLC's default is unbounded)\n"
                         "  -depth D   states per behaviour at most (default 100, as TLC)\n"
                         "  -seed S    seed of the walks (default: from the clock; printed); the generator is this "
                         "project's own, not TLC's\n", msg);
    return 150;
}

bool io_all(int fd, void *buf, size_t n, bool wr) {
    char *p = static_cast<char *>(buf);
    while (n) {
        const ssize_t k = wr ? ::write(fd, p, n) : ::read(fd, p, n);
        if (k <= 0) return false;
        p += k;
        n -= (size_t)k;
    }
    return true;
}

// -gpus N: one rank process per GPU, forked before anything touches a GPU.  Rank 0
// creates the RCCL unique id (its bootstrap root lives in that process) and sends it up a pipe;
// this process hands it down to ranks 1 .. N-1.  Rank r runs the checker on device base + r with
// world_size N (-onerank: one rank, world_size 1 with the id -- the sharded protocol through a
// one-rank communicator); only rank 0 writes TLC's output, the others' stdout goes to /dev/null.
// Returns rank 0's exit code.  A rank that dies, or ends with an error while rank 0 still runs,
// takes the others down (they would wait in a collective); after rank 0 ends the others get 60 s.
int run_ranks(int N, bool onerank, const rmc_config &base, const std::function<int(const rmc_config &)> &body) {
    std::fflush(stdout);
    std::fflush(stderr);
    int up[2];
    if (::pipe(up) != 0) { std::printf("Error: pipe failed\n"); return 75; }
    std::vector<pid_t> pid(N, -1);
    std::vector<int> down(N, -1);
    for (int r = 0; r < N; r++) {
        int p[2];
        if (::pipe(p) != 0) { std::printf("Error: pipe failed\n"); return 75; }
        const pid_t k = ::fork();
        if (k < 0) { std::printf("Error: fork failed\n"); return 75; }
        if (k == 0) {  // rank r
            ::close(p[1]);
            ::close(up[0]);
            if (r != 0) ::close(up[1]);  // (only rank 0 writes up: the others must not hold it open)
            for (int q = 0; q < r; q++) ::close(down[q]);
            // RCCL's own messages (its version line, warnings) go to stderr: stdout is TLC's
            ::setenv("NCCL_DEBUG_FILE", "/dev/stderr", 0);
            unsigned char id[128];
            if (r == 0) {
                const int rc = rmc_comm_unique_id(id);
                if (rc != RMC_OK) {
                    std::printf("Error: could not start the GPU model checker (RCCL unique id: code %d)\n", rc);
                    std::fflush(stdout);
                    std::_Exit(75);
                }
                if (!io_all(up[1], id, sizeof id, true)) std::_Exit(75);
            } else if (!io_all(p[0], id, sizeof id, false)) {
                std::_Exit(75);  // rank 0 could not start: nothing to join
            }
            if (r == 0) ::close(up[1]);
            ::close(p[0]);
            if (r != 0) {
                const int dn = ::open("/dev/null", O_WRONLY);
                if (dn >= 0) ::dup2(dn, 1);
            }
            rmc_config c = base;
            c.rank = onerank ? 0 : r;
            c.world_size = onerank ? 1 : N;
            c.comm_unique_id = id;
            c.device = (base.device >= 0 ? base.device : 0) + r;
            const int code = body(c);
            std::fflush(stdout);
            std::fflush(stderr);
            std::_Exit(code);
        }
        ::close(p[0]);
        down[r] = p[1];
        pid[r] = k;
    }
    ::close(up[1]);
    unsigned char id[128];
    const bool have = io_all(up[0], id, sizeof id, false);
    ::close(up[0]);
    for (int r = 1; r < N; r++) {
        if (have) io_all(down[r], id, sizeof id, true);
        ::close(down[r]);
    }
    ::close(down[0]);
    int code0 = 75, alive = N;
    bool rank0_done = false;
    auto kill_all = [&] {
        for (int r = 0; r < N; r++)
            if (pid[r] > 0) ::kill(pid[r], SIGKILL);
    };
    auto t_done = std::chrono::steady_clock::now();
    while (alive) {
        int st = 0;
        const pid_t w = ::waitpid(-1, &st, rank0_done ? WNOHANG : 0);
        if (w < 0) break;
        if (w == 0) {  // rank 0 has ended; the others finish their last collectives or are stopped
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_done).count() > 60.0) kill_all();
            ::usleep(100000);
            continue;
        }
        const int r = (int)(std::find(pid.begin(), pid.end(), w) - pid.begin());
        if (r >= N) continue;
        pid[r] = -1;
        alive--;
        const bool clean = WIFEXITED(st);
        const int code = clean ? WEXITSTATUS(st) : 75;
        if (r == 0) {
            code0 = code;
            rank0_done = true;
            t_done = std::chrono::steady_clock::now();
        } else if (!clean || (!rank0_done && code != 0 && code != 11 && code != 12 && code != 14)) {
            std::fprintf(stderr, "raftmc: rank %d ended (%s %d); stopping the other ranks\n", r,
                         clean ? "exit" : "signal", clean ? code : WTERMSIG(st));
            kill_all();
        }
    }
    return code0;
}

// The process that prints TLC's output is not the one whose exit frees the run's memory: run_detached
// forks one worker before anything touches a GPU; the worker prints everything, then closes its
// stdout / stderr (tee's pipe, myrun.sh:3) and reports its exit code up a pipe before it exits.  The
// kernel's teardown of the worker (~110 GB of host trace and the device memory after a Raft.cfg
// exhaustion: ~4 s) then runs after this process has returned TLC's exit code,
// so the shell returns as the "Finished" line prints.
// The worker frees the device memory itself (rmc_release_device) before it reports, so a GPU job started
// right after the shell returns finds the device free; only the host trace's teardown overlaps it.
int g_report_fd = -1;

void report(int code) {  // (a no-op in the one-process mode)
    std::fflush(stdout);
    std::fflush(stderr);
    if (g_report_fd < 0) return;
    ::close(1);  // (exit tears memory down before it closes files: tee would wait for the teardown)
    ::close(2);
    unsigned char c = (unsigned char)code;
    io_all(g_report_fd, &c, 1, true);
    ::close(g_report_fd);
    g_report_fd = -1;
}

[[noreturn]] void report_and_exit(int code) {
    report(code);
    std::_Exit(code);
}

int run_detached(const rmc_config &cfg, const std::function<int(const rmc_config &)> &body) {
    std::fflush(stdout);
    std::fflush(stderr);
    int pp[2];
    if (::pipe(pp) != 0) return body(cfg);
    const pid_t k = ::fork();
    if (k < 0) {
        ::close(pp[0]);
        ::close(pp[1]);
        return body(cfg);  // no worker: run here
    }
    if (k == 0) {
        ::close(pp[0]);
        g_report_fd = pp[1];
        report_and_exit(body(cfg));
    }
    ::close(pp[1]);
    unsigned char c = 0;
    const bool got = io_all(pp[0], &c, 1, false);
    ::close(pp[0]);
    if (got) return c;  // the worker's teardown goes on without us
    int st = 0;  // the worker ended without reporting (a crash): its status
    if (::waitpid(k, &st, 0) < 0) return 75;
    return WIFEXITED(st) ? WEXITSTATUS(st) : 75;
}

}  // namespace

// RMC_LAUNCHER_TIMES=1: seconds since process start at each phase, on stderr (stdout stays TLC's)
static const auto g_t_start = std::chrono::steady_clock::now();
static void phase_time(const char *what) {
    static const bool on = std::getenv("RMC_LAUNCHER_TIMES") && std::string(std::getenv("RMC_LAUNCHER_TIMES")) == "1";
    if (on)
        std::fprintf(stderr, "raftmc: %s at %.3f s\n", what,
                     std::chrono::duration<double>(std::chrono::steady_clock::now() - g_t_start).count());
}

int main(int argc, char **argv) {
    std::string tla_path, cfg_path;
    int check_deadlock = 1, device = -1, msgcap = 0, seenlog2 = 0, workers = 1, gpus = 1;
    bool onerank = false;                // -gpus 1 through a one-rank RCCL communicator (tests)
    unsigned long long shardmin = 0;     // -gpus: levels below this many states run replicated (0 = 2^20)
    bool print_locations = false;       // print each action's source range and exit (no GPU needed)
    double progress_s = 60.0;           // TLC reports Progress once a minute (and at the end)
    double ckpt_minutes = 30.0;         // TLC -checkpoint: minutes between checkpoints (0 = never)
    std::string metadir, recover_dir;   // TLC -metadir / -recover: where checkpoints go / come from
    bool simulate = false, ckpt_given = false, seed_given = false, sim_bad = false;  // TLC -simulate [num=N]
    unsigned long long sim_num = 1000000, sim_seed = 0;  // (TLC's -simulate is unbounded without num=)
    long long sim_depth = 100;                           // TLC -depth
    bool coverage = false, cov_bad = false;              // TLC -coverage <minutes>
    bool cont = false;                                   // TLC -continue
    bool fullstate = false;                              // -fullstate: the whole state, not the VIEW, is the identity
    bool dump = false, dump_dot = false, dump_labels = false;  // TLC -dump [dot[,options]] FILE
    std::string dump_file, dump_bad;
    std::vector<std::pair<int, int>> canreach;  // -canreach NAME[=FALSE]: (invariant bit, value)
    std::string canreach_bad;
    // -eventually NAME[=FALSE] / -leadsto Q[=FALSE] P[=FALSE]: target (bit, value), source (bit, value) or bit -1; -scc
    struct LiveQ { int bit, value, sbit, svalue; };
    std::vector<LiveQ> liveq;
    std::string live_bad, live_flag;  // the first argument that names no invariant, and its flag
    bool scc = false;
    auto inv_arg = [&](const std::string &v, int *bit, int *value) {  // NAME[=TRUE|=FALSE]
        *value = 1;
        *bit = -1;
        const size_t eq = v.find('=');
        const std::string name = v.substr(0, eq);
        if (eq != std::string::npos) {
            const std::string t = v.substr(eq + 1);
            if (t == "FALSE") *value = 0;
            else if (t != "TRUE") return false;
        }
        if (name == "LeaderHasAllCommittedEntries") *bit = 0;
        for (int b = 0; b < 7 && *bit < 0; b++)
            if (name == kInvNames[b]) *bit = b;
        return *bit >= 0;
    };
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto need = [&](const char *f) -> const char * {
            if (i + 1 >= argc) { std::fprintf(stderr, "raftmc: %s needs an argument\n", f); std::exit(150); }
            return argv[++i];
        };
        if (a == "-deadlock") check_deadlock = 0;  // TLC: -deadlock turns deadlock checking OFF
        else if (a == "-workers") workers = std::atoi(need("-workers"));  // CPU threads in TLC; the GPU path ignores it
        else if (a == "-config") cfg_path = need("-config");
        else if (a == "-device") device = std::atoi(need("-device"));
        else if (a == "-gpus") gpus = std::atoi(need("-gpus"));
        else if (a == "-onerank") onerank = true;
        else if (a == "-shardmin") shardmin = std::strtoull(need("-shardmin"), nullptr, 10);
        else if (a == "-msgcap") msgcap = std::atoi(need("-msgcap"));
        else if (a == "-seenlog2") seenlog2 = std::atoi(need("-seenlog2"));
        else if (a == "-checkpoint") { ckpt_minutes = std::atof(need("-checkpoint")); ckpt_given = true; }
        else if (a == "-simulate") {
            simulate = true;
            if (i + 1 < argc && std::strchr(argv[i + 1], '=')) {  // num=N
                const std::string v = argv[++i];
                char *end = nullptr;
                const bool digits = v.size() > 4 && v.compare(0, 4, "num=") == 0 && isdigit((unsigned char)v[4]);
                sim_num = digits ? std::strtoull(v.c_str() + 4, &end, 10) : 0;
                if (!digits || *end || sim_num == 0) sim_bad = true;
            }
        } else if (a == "-coverage") {
            coverage = true;
            char *end = nullptr;
            if (i + 1 >= argc || !isdigit((unsigned char)argv[i + 1][0])) cov_bad = true;
            else if (std::strtod(argv[++i], &end), *end) cov_bad = true;
        } else if (a == "-continue") cont = true;
        else if (a == "-fullstate") fullstate = true;
        else if (a == "-dump") {
            dump = true;
            std::string v = need("-dump");
            if (v == "dot" || v.compare(0, 4, "dot,") == 0) {  // the format and its options, then the file
                dump_dot = true;
                std::stringstream opts(v.size() > 4 ? v.substr(4) : std::string());
                for (std::string o; std::getline(opts, o, ',');) {
                    if (o == "actionlabels") dump_labels = true;
                    else dump_bad += (dump_bad.empty() ? "" : ", ") + o;
                }
                v = need("-dump dot");
            }
            dump_file = v;
        }
        else if (a == "-canreach") {
            std::string v = need("-canreach");
            int value = 1;
            const size_t eq = v.find('=');
            std::string name = v.substr(0, eq);
            if (eq != std::string::npos) {
                const std::string t = v.substr(eq + 1);
                if (t == "FALSE") value = 0;
                else if (t != "TRUE") canreach_bad = v;
            }
            int bit = -1;
            if (name == "LeaderHasAllCommittedEntries") bit = 0;
            for (int b = 0; b < 7 && bit < 0; b++)
                if (name == kInvNames[b]) bit = b;
            if (bit < 0 && canreach_bad.empty()) canreach_bad = v;
            canreach.push_back({bit, value});
        }
        else if (a == "-eventually") {
            const std::string v = need("-eventually");
            LiveQ q{-1, 1, -1, 1};
            if (!inv_arg(v, &q.bit, &q.value) && live_bad.empty()) { live_bad = v; live_flag = a; }
            liveq.push_back(q);
        }
        else if (a == "-leadsto") {
            auto is_tla = [](const char *s) { const size_t k = std::strlen(s); return k > 4 && std::strcmp(s + k - 4, ".tla") == 0; };
            if (i + 2 >= argc || argv[i + 1][0] == '-' || argv[i + 2][0] == '-' || is_tla(argv[i + 1]) || is_tla(argv[i + 2]))
                return usage("-leadsto takes two arguments: Q[=FALSE] P[=FALSE] (from a state where Q holds, P must follow)");
            const std::string qs = argv[++i], ps = argv[++i];
            LiveQ q{-1, 1, -1, 1};
            if (!inv_arg(qs, &q.sbit, &q.svalue) && live_bad.empty()) { live_bad = qs; live_flag = a; }
            if (!inv_arg(ps, &q.bit, &q.value) && live_bad.empty()) { live_bad = ps; live_flag = a; }
            liveq.push_back(q);
        }
        else if (a == "-scc") scc = true;
        else if (a == "-depth") sim_depth = std::atoll(need("-depth"));
        else if (a == "-seed") { sim_seed = (unsigned long long)std::strtoll(need("-seed"), nullptr, 10); seed_given = true; }
        else if (a == "-metadir") metadir = need("-metadir");
        else if (a == "-recover") recover_dir = need("-recover");
        else if (a == "-progress") progress_s = std::atof(need("-progress"));
        else if (a == "-print-locations") print_locations = true;
        else if (a.size() > 4 && a.compare(a.size() - 4, 4, ".tla") == 0) tla_path = a;
        else if (a[0] != '-' && tla_path.empty()) tla_path = a + ".tla";
        else return usage(("unsupported option " + a).c_str());
    }
    if (coverage) {  // refused before anything touches a device
        if (cov_bad) return usage("-coverage takes a number of minutes");
        if (simulate) return usage("-coverage cannot be combined with -simulate");
        if (!recover_dir.empty()) return usage("-coverage cannot be combined with -recover (checkpoints do not carry it)");
    }
    if (fullstate && simulate)  // refused before anything touches a device
        return usage("-fullstate cannot be combined with -simulate (random walks keep no set of states)");
    if (cont) {  // refused before anything touches a device
        if (simulate) return usage("-continue cannot be combined with -simulate");
        if (!recover_dir.empty()) return usage("-continue cannot be combined with -recover (checkpoints do not carry the violation counts)");
    }
    if (dump) {  // refused before anything touches a device
        if (!dump_bad.empty()) return usage(("-dump dot supports only the actionlabels option, not " + dump_bad).c_str());
        if (dump_file.empty() || dump_file[0] == '-') return usage("-dump takes a file name");
        if (simulate) return usage("-dump cannot be combined with -simulate");
        if (!recover_dir.empty()) return usage("-dump cannot be combined with -recover (checkpoints do not carry the state graph)");
        if (gpus > 1 || onerank) return usage("-dump runs on one GPU (no -gpus)");
        const std::string ext = dump_dot ? ".dot" : ".dump";  // (TLC appends the extension unless it is there)
        if (dump_file.size() < ext.size() || dump_file.compare(dump_file.size() - ext.size(), ext.size(), ext) != 0)
            dump_file += ext;
    }
    if (!canreach.empty()) {  // refused before anything touches a device
        if (!canreach_bad.empty())
            return usage(("-canreach " + canreach_bad + ": NAME[=TRUE|=FALSE] with NAME one of Inv, NoSplitVote, RaftCanCommt, "
                          "FollowerCanCommit, CommitAll, NoAllCommit, ExistLeaderAndCandidate").c_str());
        if (simulate) return usage("-canreach cannot be combined with -simulate");
        if (!recover_dir.empty()) return usage("-canreach cannot be combined with -recover (checkpoints do not carry the state graph)");
        if (gpus > 1 || onerank) return usage("-canreach runs on one GPU (no -gpus)");
    }
    if (!liveq.empty() || scc) {  // refused before anything touches a device
        const std::string f = !live_flag.empty() ? live_flag : !liveq.empty() ? (liveq[0].sbit >= 0 ? "-leadsto" : "-eventually") : "-scc";
        if (!live_bad.empty())
            return usage((live_flag + " " + live_bad + ": NAME[=TRUE|=FALSE] with NAME one of Inv, NoSplitVote, RaftCanCommt, "
                          "FollowerCanCommit, CommitAll, NoAllCommit, ExistLeaderAndCandidate").c_str());
        if (simulate) return usage((f + " cannot be combined with -simulate").c_str());
        if (!recover_dir.empty()) return usage((f + " cannot be combined with -recover (checkpoints do not carry the state graph)").c_str());
        if (gpus > 1 || onerank) return usage((f + " runs on one GPU (no -gpus)").c_str());
    }
    const bool keep_graph = !canreach.empty() || !liveq.empty() || scc;  // the analyses after the search need the graph
    if (simulate) {  // refused before anything touches a device
        if (sim_bad) return usage("-simulate takes num=N with N >= 1");
        if (sim_depth < 1 || sim_depth > 0x7FFFFFFFll) return usage("-depth must be at least 1");
        if (gpus > 1 || onerank) return usage("-simulate runs on one GPU (no -gpus)");
        if (!recover_dir.empty()) return usage("-simulate cannot be combined with -recover");
        if (ckpt_given) return usage("-simulate cannot be combined with -checkpoint");
        if (!seed_given)
            sim_seed = (unsigned long long)std::chrono::system_clock::now().time_since_epoch().count();
    }
    if (tla_path.empty()) return usage("missing spec file");
    if (gpus < 1 || gpus > 64) return usage("-gpus must be 1..64");
    if (cfg_path.empty()) cfg_path = tla_path.substr(0, tla_path.size() - 4) + ".cfg";
    std::string tla, cfgtxt;
    const bool skip_spec = std::getenv("RMC_SKIP_SPEC_CHECK") && std::string(std::getenv("RMC_SKIP_SPEC_CHECK")) == "1";
    if (!read_file(tla_path, &tla)) {
        if (!skip_spec) { std::fprintf(stderr, "Error: cannot read %s\n", tla_path.c_str()); return 150; }
        tla.clear();
    }
    if (print_locations) {
        // the "<Action line L, col C to line L', col C' of module M>" ranges the trace headers use
        std::vector<std::string> names(kActionNames, kActionNames + 13);
        names.insert(names.end(), kBfNames, kBfNames + 3);
        std::vector<Loc> locs = action_locations(tla, names);
        for (size_t a = 0; a < names.size(); a++)
            std::printf("%s %d %d %d %d\n", names[a].c_str(), locs[a].l0, locs[a].c0, locs[a].l1, locs[a].c1);
        return 0;
    }
    if (!read_file(cfg_path, &cfgtxt)) { std::fprintf(stderr, "Error: cannot read %s\n", cfg_path.c_str()); return 151; }
    rmc::ParsedModel pm;
    std::string err;
    if (!rmc::parse_model(cfgtxt, skip_spec ? nullptr : tla.c_str(), &pm, err)) {
        std::fprintf(stdout, "Error: %s\n", err.c_str());
        return err.rfind("cfg", 0) == 0 || err.rfind("CONSTANT", 0) == 0 ? 151 : 150;
    }
    if (skip_spec) {
        const std::string base = tla_path.substr(tla_path.find_last_of('/') + 1);
        if (base == "RaftSeeded.tla") { pm.cfg.spec_variant = RMC_SPEC_SEEDED; pm.module = "RaftSeeded"; }
        if (base == "RaftSplitBrain.tla") { pm.cfg.spec_variant = RMC_SPEC_SPLIT_BRAIN; pm.module = "RaftSplitBrain"; }
        if (base == "RaftCommitPastLog.tla") { pm.cfg.spec_variant = RMC_SPEC_COMMIT_PAST_LOG; pm.module = "RaftCommitPastLog"; }
    }
    if (pm.check_deadlock_cfg >= 0 && check_deadlock) check_deadlock = pm.check_deadlock_cfg;
    rmc_config cfg = pm.cfg;
    cfg.check_deadlock = check_deadlock;
    cfg.device = device;
    cfg.msg_cap = msgcap;
    cfg.seen_log2 = seenlog2;
    cfg.shard_min_states = shardmin;

    std::printf("raftmc (MI355X-native model checker for kikimo/tla-raft) -- TLC-compatible output\n");
    if (simulate)
        std::printf("Running Random Simulation with seed %llu on 1 GPU (%llu behaviours of at most %lld states; the "
                    "generator is raftmc's own, not TLC's).\n", sim_seed, sim_num, sim_depth);
    else
        std::printf("Running breadth-first search Model-Checking on %d GPU%s (TLC -workers %d order: 1).\n", gpus,
                    gpus > 1 ? "s" : "", workers);
    std::printf("Parsing file %s\n", tla_path.c_str());
    std::printf("Semantic processing of module %s\n", pm.module.c_str());
    for (const auto &c : pm.ignored_constants) std::printf("(ignoring assignment to undeclared constant %s)\n", c.c_str());
    std::printf("Starting... (%s)\n", now_str().c_str());
    if (fullstate) std::printf("Fingerprinting the whole state: the cfg's VIEW view is not applied.\n");
    // TLC's error lines and "The behavior up to this point is:" block for the context's trace; returns
    // TLC's exit code for the status
    // the name the cfg used for an invariant (Inv and LeaderHasAllCommittedEntries share bit 0)
    auto inv_name = [&](int bit) -> std::string {
        std::string name = kInvNames[bit];
        for (const std::string &n : pm.invariant_names)
            if ((bit == 0 && (n == "Inv" || n == "LeaderHasAllCommittedEntries")) || n == kInvNames[bit]) name = n;
        return name;
    };
    // a behaviour read out of the context (rmc_trace_state), kept while the context's current trace changes
    struct Step { std::vector<int32_t> buf; int32_t a, s, w; };
    auto read_trace = [&](void *ctx, uint32_t trace_len) {
        std::vector<Step> out;
        for (uint32_t i = 0; i < trace_len; i++) {
            Step st{std::vector<int32_t>(RMC_UNPACKED_INTS(5, 3, 256)), 0, 0, 0};
            if (rmc_trace_state(ctx, i, st.buf.data(), st.buf.size(), &st.a, &st.s, &st.w) < 0) break;
            out.push_back(std::move(st));
        }
        return out;
    };
    // "<Action line .. of module M>" of the step (a, s) taken from the state `from` (unpacked: vf, ct, role)
    auto action_title = [&](int32_t a, int32_t s, const int32_t *from, const rmc_config &cfg) -> std::string {
        static std::vector<std::string> names;
        static std::vector<Loc> locs;
        if (names.empty()) {
            names.assign(kActionNames, kActionNames + 13);
            names.insert(names.end(), kBfNames, kBfNames + 3);  // 13..15
            locs = action_locations(tla, names);
        }
        const int an = (a == 12 && s >= 0 && s < cfg.n_servers) ? 13 + (from ? from[2 * cfg.n_servers + s] : 0) : a;  // role: 0 F, 1 C, 2 L
        const Loc &L = locs[an];
        char buf[256];
        if (L.l0)
            std::snprintf(buf, sizeof buf, "<%s line %d, col %d to line %d, col %d of module %s>", names[an].c_str(), L.l0, L.c0,
                          L.l1, L.c1, pm.module.c_str());
        else
            std::snprintf(buf, sizeof buf, "<%s(%s)>", names[an].c_str(), pm.servers[s].c_str());
        return buf;
    };
    auto print_behavior = [&](const std::vector<Step> &steps, const rmc_config &cfg) {
        Printer pr{pm, cfg.n_servers, cfg.n_vals};
        for (uint32_t i = 0; i < (uint32_t)steps.size(); i++) {
            const std::vector<int32_t> &buf = steps[i].buf;
            const int32_t a = steps[i].a, s = steps[i].s;
            if (a < 0) std::printf("State %u: <Initial predicate>\n", i + 1);
            else std::printf("State %u: %s\n", i + 1, action_title(a, s, i ? steps[i - 1].buf.data() : nullptr, cfg).c_str());
            std::printf("%s\n", pr.state(buf.data()).c_str());
        }
    };
    // The behaviour from Init to the explored state `gid`: its slot keys (rmc_state_path) replayed from Init
    // (Raft.tla:93-105) through rmc_successors; empty if a step does not resolve.
    auto path_steps = [&](void *ctx, const rmc_config &cfg, uint64_t gid) {
        std::vector<Step> out;
        const int n = cfg.n_servers, V = cfg.n_vals;
        uint32_t len = 0;
        std::vector<uint32_t> keys(4096);
        if (rmc_state_path(ctx, gid, keys.data(), nullptr, (uint32_t)keys.size(), &len) < 0) return out;
        const size_t stride = RMC_UNPACKED_INTS(5, 3, 256);
        Step st{std::vector<int32_t>(stride, 0), -1, 0, 0};
        int32_t *u = st.buf.data();
        for (int i = 0; i < n; i++) {
            u[i] = -1;                              // votedFor = None
            u[3 * n + i] = 1;                       // commitIndex
            u[4 * n + i] = 1;                       // Len(logs[i]): the entry (0, None)
            u[5 * n + i * (V + 1) * 2 + 1] = -1;
        }
        int32_t *m = u + 5 * n + n * (V + 1) * 2;
        for (int i = 0; i < n * n; i++) {
            m[i] = 1;          // matchIndex
            m[n * n + i] = 2;  // nextIndex
        }
        for (int v = 0; v < V; v++) m[3 * n * n + 2 + v] = -1;  // valSent = None
        out.push_back(st);
        const uint32_t cap = 1024;
        std::vector<int32_t> succ(cap * stride);
        std::vector<uint32_t> sk(cap);
        for (uint32_t i = 1; i < len; i++) {
            uint32_t cnt = 0;
            if (rmc_successors(ctx, out.back().buf.data(), succ.data(), stride, cap, sk.data(), nullptr, &cnt) != RMC_OK)
                return std::vector<Step>();
            uint32_t j = 0;
            while (j < cnt && sk[j] != keys[i]) j++;
            if (j == cnt) return std::vector<Step>();
            Step nx{std::vector<int32_t>(succ.begin() + (size_t)j * stride, succ.begin() + (size_t)(j + 1) * stride),
                    (int32_t)((keys[i] >> 16) & 0xFF), (int32_t)(keys[i] >> 24), (int32_t)(keys[i] & 0xFFFF)};
            out.push_back(std::move(nx));
        }
        return out;
    };
    auto print_error = [&](const std::vector<Step> &steps, const rmc_config &cfg, int status, int violated) -> int {
        int exit_code = 0;
        if (status == RMC_VIOLATION) {
            std::printf("Error: Invariant %s is violated.\n", inv_name(violated).c_str());
            exit_code = 12;
        } else if (status == RMC_ASSERT) {
            std::printf("Error: The first argument of Assert evaluated to FALSE; the second argument was:\n\"split brain\"\n");
            exit_code = 14;
        } else if (status == RMC_EVAL_ERROR) {
            std::printf("Error: Evaluating invariant %s failed.\nAttempted to apply a tuple to an index out of its domain "
                        "(logs[p][index], %s.tla line 499).\n", kInvNames[violated], pm.module.c_str());
            exit_code = 75;
        } else if (status == RMC_DEADLOCK) {
            std::printf("Error: Deadlock reached.\n");
            exit_code = 11;
        }
        std::printf("Error: The behavior up to this point is:\n");
        print_behavior(steps, cfg);
        return exit_code;
    };
    auto check = [&](const rmc_config &cfg) -> int {
    const auto t0 = std::chrono::steady_clock::now();
    void *ctx = nullptr;
    phase_time("create");
    // a rank's communicator set-up prints RCCL's banner on stdout: send it to stderr (stdout is TLC's)
    const int saved_out = cfg.comm_unique_id ? ::dup(1) : -1;
    if (saved_out >= 0) {
        std::fflush(stdout);
        ::dup2(2, 1);
    }
    int rc = rmc_create(&cfg, &ctx);
    if (saved_out >= 0) {
        std::fflush(stdout);
        ::dup2(saved_out, 1);
        ::close(saved_out);
    }
    phase_time("created");
    if (rc != RMC_OK) { std::printf("Error: could not start the GPU model checker (code %d): %s\n", rc, rmc_last_error(nullptr)); return 75; }
    rmc_level_stats st;
    if (fullstate && rmc_set_full_state(ctx, 1) < 0) {
        std::printf("Error: %s\n", rmc_last_error(ctx));
        rmc_destroy(ctx);
        return 75;
    }
    if (coverage && rmc_set_coverage(ctx, 1) < 0) {
        std::printf("Error: %s\n", rmc_last_error(ctx));
        rmc_destroy(ctx);
        return 75;
    }
    if (cont && rmc_set_continue(ctx, 1) < 0) {
        std::printf("Error: %s\n", rmc_last_error(ctx));
        rmc_destroy(ctx);
        return 75;
    }
    if (keep_graph && rmc_set_graph_keep(ctx, 1) < 0) {
        std::printf("Error: %s\n", rmc_last_error(ctx));
        rmc_destroy(ctx);
        return 75;
    }
    DumpSink ds;
    const Printer dump_pr{pm, cfg.n_servers, cfg.n_vals};
    if (dump) {
        ds.path = dump_file;
        ds.dot = dump_dot;
        ds.labels = dump_labels;
        ds.pr = &dump_pr;
        rmc_graph_sink gs{};
        gs.user = &ds;
        gs.states = &DumpSink::on_states;
        gs.edges = &DumpSink::on_edges;
        if (!ds.open()) {
            std::printf("Error: %s\n", ds.err.c_str());
            rmc_destroy(ctx);
            return 75;
        }
        if (rmc_set_graph(ctx, &gs) < 0) {
            std::printf("Error: %s\n", rmc_last_error(ctx));
            rmc_destroy(ctx);
            return 75;
        }
    }
    if (!recover_dir.empty()) {
        // TLC -recover: carry on from the checkpoint in that directory (rmc_resume)
        const std::string f = recover_dir + "/raftmc.ckpt";
        std::printf("Starting recovery from checkpoint %s\n", recover_dir.c_str());
        rc = rmc_resume(ctx, f.c_str());
        if (rc < 0) { std::printf("Error: %s\n", rmc_last_error(ctx)); rmc_destroy(ctx); return 75; }
        rmc_result r0;
        rmc_get_result(ctx, &r0);
        std::printf("Recovery completed. %llu states examined. %llu states on queue.\n",
                    (unsigned long long)r0.distinct, (unsigned long long)r0.queue);
        if (metadir.empty()) metadir = recover_dir;
        rc = r0.status;
    } else {
        std::printf("Computing initial states...\n");
        rc = rmc_init(ctx, &st);
        if (rc < 0) {
            std::printf("Error: %s\n", !ds.err.empty() ? ds.err.c_str() : rmc_last_error(ctx));
            rmc_destroy(ctx);
            return 75;
        }
        std::printf("Finished computing initial states: 1 distinct state generated at %s.\n", now_str().c_str());
    }
    if (metadir.empty()) metadir = "states/" + stamp_str();
    auto last_ckpt = std::chrono::steady_clock::now();
    double gpu_seconds = 0;
    std::vector<rmc_level_stats> lv(65);
    // TLC prints Progress at start, then once per reporting interval, then at the end of the search
    auto progress = [&](const rmc_level_stats &q) {
        const double el = std::max(1e-9, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        std::printf("Progress(%d) at %s: %llu states generated (%.0f s/min), %llu distinct states found (%.0f ds/min), "
                    "%llu states left on queue.\n",
                    q.level + 1, now_str().c_str(), (unsigned long long)q.total_generated,
                    q.total_generated / el * 60.0, (unsigned long long)q.total_distinct,
                    q.total_distinct / el * 60.0, (unsigned long long)q.queue);
        std::fflush(stdout);
    };
    auto last_progress = std::chrono::steady_clock::now();
    bool reported = false, have_last = false;
    int printed_level = -1;  // the level of the last Progress line
    rmc_level_stats last{};
    while (rc == RMC_OK) {
        uint32_t nl = 0;
        rc = rmc_steps(ctx, lv.data(), (uint32_t)lv.size(), &nl);
        if (rc < 0) break;
        for (uint32_t i = 0; i < nl; i++) gpu_seconds += lv[i].seconds;
        if (nl == 0) continue;
        last = lv[nl - 1];
        have_last = true;
        const auto now = std::chrono::steady_clock::now();
        // (-dump runs a level per call where the plain run's first call covers a device-driven batch of them: its
        // first report waits for the interval or the closing one, so both runs print the same lines)
        if ((!reported && !dump && !keep_graph) ||std::chrono::duration<double>(now - last_progress).count() >= progress_s) {
            progress(last);
            reported = true;
            printed_level = last.level;
            last_progress = now;
        }
        const double since = std::chrono::duration<double>(std::chrono::steady_clock::now() - last_ckpt).count();
        if (rc == RMC_OK && ckpt_minutes > 0 && since >= ckpt_minutes * 60.0) {
            // TLC -checkpoint: the run so far, between two levels (rmc_checkpoint)
            std::printf("Checkpointing of run %s\n", metadir.c_str());
            std::error_code ec;
            std::filesystem::create_directories(metadir, ec);  // TLC's states/ metadir (no shell)
            if (ec) std::fprintf(stderr, "raftmc: cannot create %s: %s\n", metadir.c_str(), ec.message().c_str());
            const std::string f = metadir + "/raftmc.ckpt";
            if (rmc_checkpoint(ctx, f.c_str()) < 0) std::printf("Warning: checkpoint failed: %s\n", rmc_last_error(ctx));
            else std::printf("Checkpointing completed at (%s)\n", now_str().c_str());
            last_ckpt = std::chrono::steady_clock::now();
        }
    }
    if (rc < 0) {
        std::printf("Error: %s\n", !ds.err.empty() ? ds.err.c_str() : rmc_last_error(ctx));
        rmc_destroy(ctx);
        return 75;
    }
    if (dump && !ds.finish()) {
        std::printf("Error: %s\n", ds.err.c_str());
        rmc_destroy(ctx);
        return 75;
    }
    if (have_last && last.level != printed_level) progress(last);  // the closing report (once)
    rmc_result res;
    rmc_get_result(ctx, &res);
    int exit_code = 0;
    bool violations = false;
    // the stopping error's behaviour, read before the violation blocks replace the context's current trace
    const std::vector<Step> err_steps = res.status == RMC_DONE ? std::vector<Step>() : read_trace(ctx, res.trace_len);
    if (cont) {
        // -continue: per violated invariant, in cfg order, TLC's error block for the first violating
        // behaviour and the number of states that violate it (TLC prints a behaviour per state; a search
        // that can meet a hundred million of them prints one and counts the rest)
        rmc_violations vs;
        if (rmc_get_violations(ctx, &vs) < 0) std::printf("Error: no violation counts: %s\n", rmc_last_error(ctx));
        else
            for (uint32_t o = cfg.invariant_order; o; o >>= 4) {
                const int b = (int)(o & 15u) - 1;
                if (!vs.count[b]) continue;
                violations = true;
                uint32_t tl = 0;
                if (rmc_violation_trace(ctx, (uint32_t)b) < 0 || rmc_trace_len(ctx, &tl) < 0) {
                    std::printf("Error: %s\n", rmc_last_error(ctx));
                    continue;
                }
                print_error(read_trace(ctx, tl), cfg, RMC_VIOLATION, b);
                std::printf("Invariant %s is violated by %llu distinct states (first at depth %d; the first behaviour is "
                            "shown).\n", inv_name(b).c_str(), (unsigned long long)vs.count[b], vs.first_level[b]);
            }
        if (violations) exit_code = 12;
    }
    if (res.status == RMC_DONE) {
        if (!violations) std::printf("Model checking completed. No error has been found.\n");
    } else {
        exit_code = print_error(err_steps, cfg, res.status, res.violated);
    }
    // -canreach: one line per query over the graph of the search (what -dump writes), then the first state that cannot
    for (const auto &cq : canreach) {
        rmc_reach_query q{(uint32_t)cq.first, cq.second};
        rmc_reach_result rr;
        if (rmc_graph_reach(ctx, &q, &rr, nullptr) < 0) {
            std::printf("Error: no reachability of %s: %s\n", kInvNames[cq.first], rmc_last_error(ctx));
            continue;
        }
        const std::string init_d = rr.init_distance < 0 ? std::string("cannot") : std::to_string(rr.init_distance) + " steps";
        std::printf("Reachability of %s = %s: %llu of %llu distinct states satisfy it, %llu can reach one (farthest: %d steps, "
                    "Init: %s), %llu cannot", kInvNames[cq.first], cq.second ? "TRUE" : "FALSE", (unsigned long long)rr.targets,
                    (unsigned long long)rr.states, (unsigned long long)rr.can_reach, rr.max_distance, init_d.c_str(),
                    (unsigned long long)rr.cannot_reach);
        if (rr.cannot_reach) std::printf(" (first at depth %d).\n", rr.first_cannot_level);
        else std::printf(".\n");
        if (rr.cannot_reach) {
            const std::vector<Step> steps = path_steps(ctx, cfg, rr.first_cannot);
            if (steps.empty()) std::printf("Error: no behaviour to state %llu: %s\n", (unsigned long long)rr.first_cannot, rmc_last_error(ctx));
            else {
                std::printf("The behavior up to the first state that cannot is:\n");
                print_behavior(steps, cfg);
            }
        }
    }
    if (!canreach.empty()) {
        struct rmc_graph_shape gsh;
        if (rmc_graph_shape(ctx, &gsh) < 0) std::printf("Error: no graph shape: %s\n", rmc_last_error(ctx));
        else if (!gsh.cyclic_states) std::printf("The state graph has no cycle other than self-loops.\n");
        else std::printf("The state graph has %llu states on or leading to cycles.\n", (unsigned long long)gsh.cyclic_states);
    }
    // -eventually / -leadsto: one line per query; when the property fails, the behaviour to the first (source) avoider
    // and the avoid walk from it.  Every state printed is its class's stored member (path_steps replays it from Init);
    // a step's action is that of the first successor of the member with the next member's fingerprint.
    for (const LiveQ &lq : liveq) {
        rmc_live_query q{(uint32_t)lq.bit, lq.value, lq.sbit, lq.svalue};
        rmc_live_result lr;
        const std::string what = std::string(kInvNames[lq.bit]) + " = " + (lq.value ? "TRUE" : "FALSE");
        if (rmc_graph_eventually(ctx, &q, &lr, nullptr) < 0) {
            std::printf("Error: no inevitability of %s: %s\n", kInvNames[lq.bit], rmc_last_error(ctx));
            continue;
        }
        const bool leads = lq.sbit >= 0;
        const std::string init_w = lr.init_within < 0 ? std::string("Init can avoid it") : "Init: " + std::to_string(lr.init_within) + " steps";
        if (leads)
            std::printf("Leads-to %s = %s ~> %s: %llu of %llu distinct states satisfy the first, %llu of them can avoid the second "
                        "forever%s; ", kInvNames[lq.sbit], lq.svalue ? "TRUE" : "FALSE", what.c_str(), (unsigned long long)lr.sources,
                        (unsigned long long)lr.states,
                        (unsigned long long)lr.source_avoiders,
                        lr.source_avoiders ? (" (first at depth " + std::to_string(lr.first_source_avoid_level) + ")").c_str() : "");
        else
            std::printf("Inevitability of %s: ", what.c_str());
        std::printf("%llu of %llu distinct states satisfy it, %llu must reach one (latest: %d steps, %s), %llu can avoid it forever",
                    (unsigned long long)lr.targets, (unsigned long long)lr.states, (unsigned long long)lr.must, lr.max_within,
                    init_w.c_str(), (unsigned long long)lr.avoiders);
        if (lr.avoiders)
            std::printf(" (first at depth %d; %llu of them end where no step leads out).\n", lr.first_avoid_level,
                        (unsigned long long)lr.avoid_terminal);
        else std::printf(".\n");
        const bool fails = leads ? lr.source_avoiders > 0 : lr.init_within < 0;
        if (!fails) continue;
        std::printf("Error: Temporal properties were violated.\n");
        std::printf("Error: The following behavior constitutes a counter-example:\n");
        const uint64_t from = leads ? lr.first_source_avoid : lr.first_avoid;  // (-eventually: Init, gid 0)
        std::vector<uint64_t> walk(4096);
        uint32_t wl = 0;
        int32_t loop_at = -1;
        int wrc = rmc_graph_avoid_path(ctx, from, walk.data(), (uint32_t)walk.size(), &wl, &loop_at);
        if (wrc < 0 && wl > walk.size()) {
            walk.resize(wl);
            wrc = rmc_graph_avoid_path(ctx, from, walk.data(), (uint32_t)walk.size(), &wl, &loop_at);
        }
        std::vector<Step> steps = wrc < 0 ? std::vector<Step>() : path_steps(ctx, cfg, from);
        if (steps.empty()) {
            std::printf("Error: no behaviour from state %llu: %s\n", (unsigned long long)from, rmc_last_error(ctx));
            continue;
        }
        const size_t stem = steps.size() - 1;  // the walk's state i is state stem + i of the behaviour
        const size_t stride = RMC_UNPACKED_INTS(5, 3, 256);
        const uint32_t cap = 1024;
        std::vector<int32_t> succ(cap * stride);
        std::vector<uint32_t> sk(cap);
        std::vector<uint64_t> sfp(2 * (size_t)cap);
        // the key of the first successor of `a` whose fingerprint is b's; false if there is none
        auto step_key = [&](const std::vector<int32_t> &a, const std::vector<int32_t> &b, uint32_t *key) {
            uint32_t cnt = 0;
            uint64_t fp[2];
            if (rmc_fingerprint(ctx, b.data(), fp) != RMC_OK) return false;
            if (rmc_successors(ctx, a.data(), succ.data(), stride, cap, sk.data(), sfp.data(), &cnt) != RMC_OK) return false;
            for (uint32_t j = 0; j < cnt; j++)
                if (sfp[2 * j] == fp[0] && sfp[2 * j + 1] == fp[1]) {
                    *key = sk[j];
                    return true;
                }
            return false;
        };
        bool ok = true;
        for (uint32_t i = 1; i < wl && ok; i++) {
            std::vector<Step> member = path_steps(ctx, cfg, walk[i]);
            uint32_t key = 0;
            ok = !member.empty() && step_key(steps.back().buf, member.back().buf, &key);
            if (ok) steps.push_back(Step{member.back().buf, (int32_t)((key >> 16) & 0xFF), (int32_t)(key >> 24), (int32_t)(key & 0xFFFF)});
        }
        uint32_t back_key = 0;
        if (ok && loop_at >= 0) ok = step_key(steps.back().buf, steps[stem + loop_at].buf, &back_key);
        if (!ok) {
            std::printf("Error: the behaviour from state %llu does not resolve: %s\n", (unsigned long long)from, rmc_last_error(ctx));
            continue;
        }
        print_behavior(steps, cfg);
        if (loop_at < 0) std::printf("State %zu: Stuttering\n", steps.size() + 1);
        else
            std::printf("Back to state %zu: %s\n", stem + loop_at + 1,
                        action_title((int32_t)((back_key >> 16) & 0xFF), (int32_t)(back_key >> 24), steps.back().buf.data(), cfg).c_str());
    }
    if (scc) {
        rmc_scc_result sr;
        if (rmc_graph_scc(ctx, &sr, nullptr) < 0) std::printf("Error: no components: %s\n", rmc_last_error(ctx));
        else
            std::printf("The state graph has %llu strongly connected components: %llu of more than one state (%llu states, the "
                        "largest %llu).\n", (unsigned long long)sr.components, (unsigned long long)sr.nontrivial,
                        (unsigned long long)sr.nontrivial_states, (unsigned long long)sr.largest);
    }
    rmc_coverage cov;
    const int cov_rc = coverage && cfg.rank == 0 ? rmc_get_coverage(ctx, &cov) : RMC_OK;
    if (cov_rc < 0) std::printf("Error: no coverage statistics: %s\n", rmc_last_error(ctx));
    if (coverage && cfg.rank == 0 && cov_rc == RMC_OK) {
        // TLC's end-of-run coverage block, one line per disjunct of Next in textual order with the ranges
        // the trace headers use.  BecomeFollower (tla:420 variant) is one line here; TLC would report its
        // three disjuncts apart.  FollowerAppendEntry is not in Next.
        std::vector<std::string> names(kActionNames, kActionNames + 13);
        names.push_back("Init");
        const std::vector<Loc> locs = action_locations(tla, names);
        auto line = [&](int a, unsigned long long d, unsigned long long g) {
            const Loc &L = locs[a];
            if (L.l0)
                std::printf("<%s line %d, col %d to line %d, col %d of module %s>: %llu:%llu\n", names[a].c_str(), L.l0,
                            L.c0, L.l1, L.c1, pm.module.c_str(), d, g);
            else
                std::printf("<%s>: %llu:%llu\n", names[a].c_str(), d, g);
        };
        std::printf("The coverage statistics at %s\n", now_str().c_str());
        line(13, (unsigned long long)cov.init_distinct, (unsigned long long)cov.init_generated);
        static const int order[12] = {0, 1, 12, 2, 3, 4, 5, 6, 7, 8, 9, 10};  // Next's order; 12 = BecomeFollower
        for (int a : order) {
            if (a == 12 && cfg.spec_variant != RMC_SPEC_BECOME_FOLLOWER) continue;
            line(a, (unsigned long long)cov.distinct[a], (unsigned long long)cov.generated[a]);
        }
        std::printf("End of statistics.\n");
    }
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("%llu states generated, %llu distinct states found, %llu states left on queue.\n",
                (unsigned long long)res.generated, (unsigned long long)res.distinct, (unsigned long long)res.queue);
    if (res.status == RMC_DONE)
        std::printf("The depth of the complete state graph search is %d.\n", res.depth);
    std::printf("Finished in %.2fs at (%s)\n", el, now_str().c_str());
    std::printf("GPU: %.0f distinct states/s over %.3f s of BFS levels (MI355X, %d device%s).\n",
                gpu_seconds > 0 ? res.distinct / gpu_seconds : 0.0, gpu_seconds, cfg.world_size > 1 ? cfg.world_size : 1,
                cfg.world_size > 1 ? "s" : "");
    // The process ends here: by default the device and host memory (~250 GB and ~110 GB of
    // trace at Raft.cfg) go back with the process instead of through rmc_destroy, whose frees took
    // ~16 s after a Raft.cfg exhaustion (RMC_FAST_EXIT=0 destroys the context first).
    std::fflush(stdout);
    std::fflush(stderr);
    const char *fe = std::getenv("RMC_FAST_EXIT");
    if (!(fe && std::string(fe) == "0")) {
        if (g_report_fd >= 0) {  // detached worker: the device goes back before the caller has its code
            phase_time("release device");
            rmc_release_device(ctx);
            phase_time("device released");
            report(exit_code);
        }
        std::_Exit(exit_code);
    }
    phase_time("destroy");
    rmc_destroy(ctx);
    phase_time("destroyed");
    return exit_code;
    };
    // -simulate: seeded random behaviours (rmc_simulate) instead of the search
    auto sim = [&](const rmc_config &cfg) -> int {
        const auto t0 = std::chrono::steady_clock::now();
        void *ctx = nullptr;
        int rc = rmc_create(&cfg, &ctx);
        if (rc != RMC_OK) { std::printf("Error: could not start the GPU model checker (code %d): %s\n", rc, rmc_last_error(nullptr)); return 75; }
        rmc_sim_config sc{};
        sc.num_walks = sim_num;
        sc.seed = sim_seed;
        sc.depth = (uint32_t)sim_depth;
        rmc_sim_result sr{};
        rc = rmc_simulate(ctx, &sc, &sr, nullptr, nullptr);
        if (rc < 0) {
            std::printf("Error: %s\n", rmc_last_error(ctx));
            rmc_destroy(ctx);
            return 75;
        }
        int exit_code = 0;
        if (sr.status == RMC_DONE) {
            std::printf("Simulation completed. No error has been found.\n");
        } else {
            uint32_t tl = 0;
            rmc_trace_len(ctx, &tl);
            exit_code = print_error(read_trace(ctx, tl), cfg, sr.status, sr.violated);
            std::printf("The error is in behaviour %llu (%u states) of seed %llu.\n", (unsigned long long)sr.err_walk,
                        sr.err_len, sim_seed);
        }
        const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("Simulation using seed %llu: %llu behaviours checked (longest %u states, %llu ended in a state "
                    "without successors).\n", sim_seed, (unsigned long long)sr.walks, sr.longest,
                    (unsigned long long)sr.ended_early);
        std::printf("%llu states checked, %llu states generated.\n", (unsigned long long)sr.states,
                    (unsigned long long)sr.generated);
        std::printf("Finished in %.2fs at (%s)\n", el, now_str().c_str());
        std::printf("GPU: %.0f walk steps/s over %.3f s of walks (MI355X).\n",
                    sr.seconds > 0 ? sr.states / sr.seconds : 0.0, sr.seconds);
        std::fflush(stdout);
        std::fflush(stderr);
        rmc_destroy(ctx);
        return exit_code;
    };
    if (gpus > 1 || onerank) return run_ranks(gpus, onerank, cfg, check);
    const std::function<int(const rmc_config &)> body = simulate ? std::function<int(const rmc_config &)>(sim)
                                                                 : std::function<int(const rmc_config &)>(check);
    const char *det = std::getenv("RMC_DETACH");  // RMC_DETACH=0: one process, exit after the teardown
    if (det && std::string(det) == "0") return body(cfg);
    return run_detached(cfg, body);
}
