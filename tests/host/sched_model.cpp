// Host model of the engine's stream scheduler (csrc/sched.h; the ordering contract: DESIGN.md 3.8).
//
// Plain C++, not linked against the HIP runtime: the few runtime functions the scheduler references are defined here, as the
// definitions of record and wait.  A stream is an in-order counter (its position = kernels enqueued so far) that carries, per other
// stream, the position known to be complete at its own position.  hipEventRecord snapshots the stream's position and vector into
// the event, overwriting an older record; hipStreamWaitEvent merges the event's CURRENT snapshot into the waiting stream and is a
// no-op for a never-recorded event.  A kernel advances its stream and goes through tail_note_launch, like every launch of the library.
//
// The driver issues the call patterns of the planner's op lambdas (engine.hip) as scripted passes and seeded random interleavings
// and checks the nine points of the contract after every call.  --break=N disables one edge of the scheduler (CDRL_SCHED_BROKEN in
// sched.h: 1 the wait of a claim, 2 the record of done_side, 3 the flush of fork_side): the run must then fail.
extern int cdrl_sched_break;
#define CDRL_SCHED_BROKEN(n) (cdrl_sched_break == (n))
#include "../../carla-driving-rl-agent_amd/csrc/sched.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <set>
#include <string>

int cdrl_sched_break = 0;

// ------------------------------------------------------------------------------------------------ the runtime, as its definitions
namespace {
constexpr int MAXS = 8;
struct Clock {
    uint64_t v[MAXS] = {};
    void merge(const Clock& o) {
        for (int i = 0; i < MAXS; ++i)
            if (o.v[i] > v[i]) v[i] = o.v[i];
    }
};
struct Stream {
    int id = 0;
    uint64_t pos = 0;
    Clock seen;             // seen.v[j]: position of stream j complete before anything enqueued here from now on
    int records = 0, waits = 0;
    Clock now() const {
        Clock c = seen;
        c.v[id] = pos;
        return c;
    }
};
struct Event {
    unsigned flags = 0;
    bool recorded = false;
    Clock snap;
};
int g_streams = 0, g_live = 0, g_records = 0, g_waits = 0, g_ext = 0;
Event* g_last_recorded = nullptr;
std::map<std::string, std::string> g_env;
char g_error[512] = "";
std::string g_config;

Stream* S(hipStream_t s) { return reinterpret_cast<Stream*>(s); }
Event* E(hipEvent_t e) { return reinterpret_cast<Event*>(e); }

[[noreturn]] void fail(const char* point, const char* fmt, ...) {
    char msg[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
    printf("FAIL %s: %s [%s]\n", point, msg, g_config.c_str());
    exit(1);
}
#define CHECK(cond, point, ...) \
    do {                        \
        if (!(cond)) fail(point, __VA_ARGS__); \
    } while (0)
}  // namespace

hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned, int) {
    Stream* st = new Stream;
    st->id = g_streams++;
    if (st->id >= MAXS) fail("model", "too many streams");
    ++g_live;
    *s = reinterpret_cast<hipStream_t>(st);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s) {
    delete S(s);
    --g_live;
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned flags) {
    Event* ev = new Event;
    ev->flags = flags;
    ++g_live;
    *e = reinterpret_cast<hipEvent_t>(ev);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t e) {
    delete E(e);
    --g_live;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s) {
    E(e)->recorded = true;
    E(e)->snap = S(s)->now();
    ++S(s)->records;
    ++g_records;
    g_last_recorded = E(e);
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
    if (E(e)->recorded) S(s)->seen.merge(E(e)->snap);
    ++S(s)->waits;
    ++g_waits;
    return hipSuccess;
}
const char* hipGetErrorString(hipError_t) { return "model"; }

namespace cdrl {
thread_local TailEvents* tl_tail = nullptr;
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}
const char* last_error() { return g_error; }
const char* cdrl_getenv(const char* name) {
    auto it = g_env.find(name);
    return it == g_env.end() ? nullptr : it->second.c_str();
}
}  // namespace cdrl

// ------------------------------------------------------------------------------------------------ the driver
namespace {
using cdrl::StreamSched;
constexpr int NSLOT = StreamSched::NSLOT, NQ = StreamSched::NQ;

struct Config {
    int lag = 4;
    bool tail = true, side = true, graph = false, comm = false;
};

struct Driver {
    Config cfg;
    StreamSched sched;
    hipStream_t main = nullptr, side = nullptr, aux = nullptr, caller = nullptr, comm = nullptr, other = nullptr;
    // what the scratch holds: side position of the last job that read slot / ring entry s, and whether one ran since the last join
    uint64_t slot_reader[NSLOT] = {}, q_reader[NQ] = {};
    bool slot_used[NSLOT] = {}, q_used[NQ] = {};
    int queued = 0;                     // deferred jobs issued and not yet run
    std::set<int> queued_slots;
    uint64_t aux_done = 0;              // aux position at the last done_aux
    bool aux_pending = false;
    // tail events, as the driver expects them: per body the launches a fork followed in an earlier run
    std::map<std::vector<uint64_t>, std::set<int>> learned;
    std::vector<uint64_t> key;
    int launches = 0;                   // kernels of this body on main so far
    bool kernel_is_newest = false;      // nothing went onto main behind its newest kernel
    bool repeated = false;              // this body's op sequence ran before under the same key
    int claims = 0, claim_waits = 0;

    explicit Driver(const Config& c) : cfg(c) {
        g_env.clear();
        g_env["CDRL_SIDE_LAG"] = std::to_string(c.lag);
        if (!c.tail) g_env["CDRL_TAIL_EVENTS"] = "0";
        if (!c.side) g_env["CDRL_SIDE_STREAM"] = "0";
        if (c.graph) g_env["CDRL_GRAPH"] = "1";
        g_streams = 0;
        CHECK(sched.create() == 0 && sched.created(), "create", "%s", g_error);
        main = sched.main(), side = sched.side(), aux = sched.aux();
        for (hipStream_t* s : {&caller, &comm, &other}) (void)hipStreamCreateWithPriority(s, 0, 0);
        if (c.comm) sched.set_comm(comm);
        CHECK(sched.side_on() == c.side && sched.graphs() == c.graph, "create", "switches not read");
    }
    ~Driver() {
        for (hipStream_t s : {caller, comm, other}) (void)hipStreamDestroy(s);
    }
    bool tail_on() const { return cfg.tail && !cfg.graph; }

    // one kernel launch, as launch_tracked issues it
    void kernel(hipStream_t st) {
        hipEvent_t ev = cdrl::tail_note_launch(st);
        ++S(st)->pos;
        if (ev) {           // stop event: completes with this kernel, nothing is enqueued for it
            E(ev)->recorded = true;
            E(ev)->snap = S(st)->now();
            ++g_ext;
        }
        if (st == main) ++launches, kernel_is_newest = true;
    }
    void memset_on_main() {
        cdrl::tail_invalidate(main);
        kernel_is_newest = false;
    }
    void begin(const std::vector<uint64_t>& k, bool rep) {
        key = k, repeated = rep, launches = 0, kernel_is_newest = false;
        sched.begin_body(key);
    }
    void end() { sched.end_body(); }

    // point 2: a fork from main to `to`.  Returns the records it must put on main; the caller runs the fork between the two halves.
    struct ForkCheck { uint64_t main_pos; int records, expect; };
    ForkCheck before_fork() {
        int expect = 1;
        if (tail_on()) {
            std::set<int>& l = learned[key];
            if (kernel_is_newest && l.count(launches - 1)) expect = 0;
            else if (launches > 0) l.insert(launches - 1);
            if (repeated && kernel_is_newest) CHECK(expect == 0, "2 fork", "repeated run: launch %d was not marked", launches - 1);
        }
        kernel_is_newest = kernel_is_newest && expect == 0;       // a record went in behind the kernel
        return ForkCheck{S(main)->pos, S(main)->records, expect};
    }
    void after_fork(const ForkCheck& f, hipStream_t to, const char* what) {
        CHECK(S(to)->seen.v[S(main)->id] >= f.main_pos, "2 fork", "%s: the target stream does not see main at the fork (%llu < %llu)", what,
              (unsigned long long)S(to)->seen.v[S(main)->id], (unsigned long long)f.main_pos);
        CHECK(S(main)->records - f.records == f.expect, "2 fork", "%s: %d records on the critical stream, expected %d", what,
              S(main)->records - f.records, f.expect);
        CHECK(queued == 0, "2 fork", "%s: %d deferred jobs not flushed", what, queued);
    }

    // flush_side / join_side / publish_tail: a fork to the side stream iff jobs are queued; `extra`: the call's own records on main
    struct Flush { bool forks; ForkCheck f; };
    Flush before_flush() {
        const bool forks = cfg.side && queued > 0;
        return Flush{forks, forks ? before_fork() : ForkCheck{S(main)->pos, S(main)->records, 0}};
    }
    void after_flush(Flush x, const char* what, int extra = 0) {
        x.f.expect += extra;
        if (x.forks) {
            after_fork(x.f, side, what);
            slot_used[sched.slot()] = true;         // (the done_side behind the flush marks the current slot)
        } else {
            CHECK(S(main)->records - x.f.records == extra, "2 fork", "%s: recorded on the critical stream with nothing to flush", what);
        }
    }

    // points 1, 4: a claim
    void check_claim(hipStream_t st, int waits_before, uint64_t reader, bool used, const char* what, int s) {
        const int w = S(st)->waits - waits_before;
        CHECK(S(st)->seen.v[S(side)->id] >= reader, "1 claim", "%s %d: claimed while its last reader (side %llu) is not covered (%llu)", what, s,
              (unsigned long long)reader, (unsigned long long)S(st)->seen.v[S(side)->id]);
        if (st != main || cfg.lag < 0) CHECK(w == (used ? 1 : 0), "4 waits", "%s %d: %d waits, used = %d", what, s, w, (int)used);
        else CHECK(w <= (used ? 1 : 0), "4 waits", "%s %d: %d waits, used = %d", what, s, w, (int)used);
        claims += used ? 1 : 0, claim_waits += w;
    }
    int claim(hipStream_t st = nullptr) {
        if (!st) st = main;
        const int calls = g_records + g_waits, w0 = S(st)->waits;
        CHECK(sched.next_slot(st) == 0, "claim", "%s", g_error);
        const int s = sched.slot();
        if (!cfg.side) CHECK(g_records + g_waits == calls, "6 side off", "next_slot made a runtime call");
        else check_claim(st, w0, slot_reader[s], slot_used[s], "slot", s);
        return s;
    }
    int claim_q() {
        const int w0 = S(main)->waits;
        CHECK(sched.next_q(main) == 0, "claim", "%s", g_error);
        const int q = sched.q();
        if (cfg.side) check_claim(main, w0, q_reader[q], q_used[q], "ring entry", q);
        return q;
    }
    void side_reads(int s) {            // a side job that reads slot s is enqueued
        kernel(side);
        slot_reader[s] = S(side)->pos, slot_used[s] = true;
    }
    hipStream_t fork() {
        if (!cfg.side) {
            const int calls = g_records + g_waits;
            CHECK(sched.fork_side(main) == main && g_records + g_waits == calls, "6 side off", "fork_side did not just return its argument");
            return main;
        }
        ForkCheck f = before_fork();
        CHECK(sched.fork_side(main) == side, "2 fork", "fork_side failed");
        after_fork(f, side, "fork_side");
        return side;
    }
    // a deferred job: reads slot s (and ring entry q, released behind it) after whatever main held when it was deferred
    void defer(int s, int q = -1, int rc = 0) {
        const uint64_t main_pos = S(main)->pos;
        const int before = queued;
        ++queued, queued_slots.insert(s);
        const int r = sched.defer_side(main, [=](hipStream_t sd) -> int {
            --queued, queued_slots.erase(s);
            if (sd != main) CHECK(S(sd)->seen.v[S(main)->id] >= main_pos, "2 fork", "a flushed job does not see main at its defer");
            kernel(sd);
            if (sd == side) slot_reader[s] = S(side)->pos, slot_used[s] = true;
            if (q >= 0) {
                if (sd == side) q_reader[q] = S(side)->pos, q_used[q] = true;
                CHECK(sched.release_q(q, sd) == 0, "release_q", "%s", g_error);
            }
            return rc;
        });
        if (!cfg.side) CHECK(queued == before && r == rc, "6 side off", "defer_side did not run the job inline");
        else CHECK(queued == before + 1 && r == 0, "defer", "the job ran at once");
    }
    void flush() {
        Flush x = before_flush();
        CHECK(sched.flush_side(main) == 0, "flush", "%s", g_error);
        after_flush(x, "flush_side");
    }
    void done(hipStream_t sd) {
        CHECK(sched.done_side(sd) == 0, "done", "%s", g_error);
        if (sd == side) slot_used[sched.slot()] = true;
    }
    // the rule of every op list: a deferred job goes out before its slot comes round again
    void keep_rule() {
        if (queued_slots.count((sched.slot() + 1) % NSLOT)) flush();
    }

    // ---- the op patterns (engine.hip)
    void op_side_job(bool claims_slot) {            // dense / GRU / plain conv / stem: write on main, fork, side jobs read, done
        if (claims_slot) keep_rule();
        const int s = claims_slot ? claim() : sched.slot();
        kernel(main);
        hipStream_t sd = fork();
        if (sd == side) side_reads(s), side_reads(s);
        else kernel(sd);
        done(sd);
    }
    void op_defer() {                               // depthwise block: claim, write on main, filter partials reduced later
        keep_rule();
        const int s = claim();
        kernel(main);
        defer(s);
    }
    void op_claim_only() {                          // fused stem / BatchNorm apply into the slot: no fork
        keep_rule();
        claim();
        kernel(main);
    }
    void op_prologue(bool claims_slot) {            // filter gradient on the side stream, backward-data on main, bias sums deferred
        if (claims_slot) keep_rule();
        const int s = claims_slot ? claim() : sched.slot();
        hipStream_t sd = fork();
        if (sd == side) side_reads(s);
        else kernel(sd);
        done(sd);
        kernel(main);
        defer(s);
    }
    void op_fused(bool claims_slot, bool on_main) { // fused conv backward: ring claim, tiles on main, reduce on main or deferred + flush
        if (claims_slot) keep_rule();
        const int s = claims_slot ? claim() : sched.slot();
        const int q = claim_q();
        kernel(main);
        if (on_main) {
            kernel(main);
            return;
        }
        defer(s, q);
        flush();
    }
    void op_shortcut(int stage) {                   // forward of a stride-2 unit
        const int calls = g_records + g_waits;
        ForkCheck f = cfg.side ? before_fork() : ForkCheck{};
        CHECK(sched.fork_shortcut(main, stage) == 0, "fork", "%s", g_error);
        if (cfg.side) after_fork(f, side, "fork_shortcut");
        hipStream_t sc = cfg.side ? side : main;
        kernel(sc), kernel(main), kernel(sc), kernel(main);
        CHECK(sched.join_shortcut(main, stage) == 0, "join", "%s", g_error);
        if (cfg.side) CHECK(S(main)->seen.v[S(side)->id] >= S(side)->pos, "3 join", "join_shortcut does not cover the shortcut ops");
        else CHECK(g_records + g_waits == calls, "6 side off", "the shortcut fork / join made a runtime call");
        kernel(main);
    }
    void op_aux_fork() {                            // as the op lambdas: inline on `st` when the side stream is off
        if (!cfg.side) {
            kernel(main);
            return;
        }
        ForkCheck f = before_fork();
        CHECK(sched.fork_aux(main) == 0, "fork", "%s", g_error);
        after_fork(f, aux, "fork_aux");
        kernel(aux), kernel(aux);
        CHECK(sched.done_aux() == 0, "done", "%s", g_error);
        aux_done = S(aux)->pos, aux_pending = true;
    }
    void op_aux_join() {                            // forward only
        const int calls = g_records + g_waits;
        CHECK(sched.join_aux(main) == 0, "join", "%s", g_error);
        if (cfg.side) CHECK(S(main)->seen.v[S(aux)->id] >= aux_done, "3 join", "join_aux does not cover the aux ops");
        else CHECK(g_records + g_waits == calls, "6 side off", "join_aux made a runtime call");
        aux_pending = false;
    }
    void op_publish_tail() {                        // point 7
        const int calls = g_records + g_waits;
        const uint64_t main_pos = S(main)->pos;
        if (!cfg.comm || cfg.graph) {
            CHECK(sched.publish_tail(main) == 0, "publish", "%s", g_error);
            CHECK(g_records + g_waits == calls, "7 publish_tail", "calls without a communication stream / under graph mode");
            return;
        }
        Flush x = before_flush();
        CHECK(sched.publish_tail(main) == 0, "publish", "%s", g_error);
        after_flush(x, "publish_tail", 1);
        CHECK(!(g_last_recorded->flags & hipEventDisableSystemFence), "7 publish_tail", "the newest tail event is not fenced");
        const Clock& c = S(comm)->seen;
        CHECK(c.v[S(main)->id] >= main_pos, "7 publish_tail", "main not covered");
        if (!cfg.side) return;
        CHECK(queued == 0, "7 publish_tail", "%d queued side jobs not enqueued", queued);
        CHECK(c.v[S(side)->id] >= S(side)->pos, "7 publish_tail", "side jobs not covered");
        if (aux_pending) CHECK(c.v[S(aux)->id] >= aux_done, "7 publish_tail", "pending aux backward not covered");
    }
    void op_join() {                                // point 3: end of a backward
        const int calls = g_records + g_waits;
        Flush x = before_flush();
        CHECK(sched.join_side(main) == 0, "join", "%s", g_error);
        if (!cfg.side) {
            CHECK(g_records + g_waits == calls, "6 side off", "join_side made a runtime call");
            return;
        }
        after_flush(x, "join_side");
        CHECK(queued == 0, "3 join", "%d deferred jobs never ran", queued);
        CHECK(S(main)->seen.v[S(side)->id] >= S(side)->pos, "3 join", "side stream not covered");
        if (aux_pending) CHECK(S(main)->seen.v[S(aux)->id] >= aux_done, "3 join", "pending aux backward not covered");
        aux_pending = false;
        // every used flag is clear (check_claim holds the next claims to no wait), and every reader so far is behind the join
        for (int i = 0; i < NSLOT; ++i) slot_used[i] = false, slot_reader[i] = 0;
        for (int i = 0; i < NQ; ++i) q_used[i] = false, q_reader[i] = 0;
    }

    void forward() {
        op_aux_fork();
        kernel(main);
        for (int stage = 0; stage < 3; ++stage) op_shortcut(stage);
        op_aux_join();
        kernel(main);
    }
    // one backward in the order of a reversed op list: heads / tail, publish, aux fork, the tower's units, the stem
    void backward_scripted(int units) {
        op_side_job(true), op_side_job(true);
        op_publish_tail();
        op_side_job(true);
        op_aux_fork();
        claim(other);
        for (int u = 0; u < units; ++u) {
            op_claim_only();
            op_side_job(false);                     // plain conv reads the slot its BatchNorm left
            op_fused(true, u % 2 == 0);
            op_defer();
            if (u % 3 == 0) memset_on_main();
            op_fused(false, false);
            op_prologue(u % 2 == 1);
        }
        op_claim_only();
        op_join();
    }
    void backward_random(unsigned seed, int ops) {
        std::mt19937 rng(seed);
        op_side_job(true);
        if (rng() % 2) op_publish_tail();
        op_aux_fork();
        for (int i = 0; i < ops; ++i) {
            const unsigned r = rng() % 16;
            if (r < 3) op_side_job(rng() % 2);
            else if (r < 6) op_defer();
            else if (r < 8) op_claim_only();
            else if (r < 10) op_prologue(rng() % 2);
            else if (r < 13) op_fused(rng() % 2, rng() % 3 == 0);
            else if (r == 13) memset_on_main();
            else if (r == 14) flush();
            else claim(other);
        }
        if (rng() % 2) op_publish_tail();
        op_join();
    }
    void pass(uint64_t kind, unsigned seed, bool rep) {
        CHECK(sched.hand_in(caller) == 0, "hand_in", "%s", g_error);
        begin({kind, seed}, rep);
        forward();
        if (kind == 0) backward_scripted(40);
        else backward_random(seed, 300);
        end();
        CHECK(sched.hand_out(caller) == 0, "hand_out", "%s", g_error);
    }
};

void run_passes(const Config& c) {
    char name[128];
    snprintf(name, sizeof(name), "lag=%d tail=%d side=%d graph=%d comm=%d", c.lag, (int)c.tail, (int)c.side, (int)c.graph, (int)c.comm);
    g_config = name;
    {
        Driver d(c);
        for (int rep = 0; rep < 2; ++rep) d.pass(0, 0, rep == 1);                               // scripted: first run, repeated run
        for (unsigned seed = 1; seed <= 4; ++seed)
            for (int rep = 0; rep < 2; ++rep) d.pass(1, seed, rep == 1);                        // seeded interleavings, each twice
        d.pass(0, 0, true);
        if (c.side) CHECK(d.claims > 1000, "model", "only %d claims of a used slot: the passes do not wrap the slots", d.claims);
        if (c.side && c.lag >= 0 && c.lag < StreamSched::SIDE_HIST) CHECK(d.claim_waits < d.claims, "4 waits", "the lagged wait saved nothing (%d of %d)", d.claim_waits, d.claims);
        if (d.tail_on() && c.side) CHECK(g_ext > 0, "2 fork", "no launch ever carried a stop event");
    }
    CHECK(g_live == 0, "lifetime", "%d streams / events outlive the scheduler", g_live);
    g_ext = 0;
}

// point 5: the return code of a failing deferred job surfaces exactly once, at the next done_side / flush_side / join_side
void run_deferred_errors() {
    g_config = "deferred errors";
    for (int where = 0; where < 3; ++where) {
        Driver d(Config{});
        d.begin({9, (uint64_t)where}, false);
        const int s = d.claim();
        d.kernel(d.main);
        d.defer(s, -1, 7);
        int rc;
        if (where == 0) {
            hipStream_t sd = d.sched.fork_side(d.main);
            rc = d.sched.done_side(sd);
        } else {
            rc = where == 1 ? d.sched.flush_side(d.main) : d.sched.join_side(d.main);
        }
        CHECK(rc == 7, "5 deferred errors", "site %d returned %d, not the job's 7", where, rc);
        CHECK(d.queued == 0, "5 deferred errors", "the failing job never ran");
        hipStream_t sd = d.sched.fork_side(d.main);
        CHECK(d.sched.done_side(sd) == 0 && d.sched.flush_side(d.main) == 0 && d.sched.join_side(d.main) == 0, "5 deferred errors",
              "the code surfaced twice");
        d.end();
    }
}

// point 8: the fenced pair exactly when a communication stream is set or a scaled pass has run; nothing inside a sequence on its stream
void run_hand_over() {
    g_config = "hand-over";
    for (int mode = 0; mode < 3; ++mode) {      // 0 plain, 1 communication stream, 2 scaled pass
        Config c;
        c.comm = mode == 1;
        Driver d(c);
        if (mode == 2) d.sched.note_scaled_pass();
        const bool fenced = mode != 0;
        auto is_fenced = [] { return !(g_last_recorded->flags & hipEventDisableSystemFence); };
        d.kernel(d.caller);
        CHECK(d.sched.hand_in(d.caller) == 0, "8 hand-over", "%s", g_error);
        CHECK(is_fenced() == fenced, "8 hand-over", "hand_in: fenced = %d in mode %d", (int)is_fenced(), mode);
        CHECK(S(d.main)->seen.v[S(d.caller)->id] >= S(d.caller)->pos, "8 hand-over", "main is not behind the caller");
        d.kernel(d.main);
        CHECK(d.sched.hand_out(d.caller) == 0, "8 hand-over", "%s", g_error);
        CHECK(is_fenced() == fenced, "8 hand-over", "hand_out: fenced = %d in mode %d", (int)is_fenced(), mode);
        CHECK(S(d.caller)->seen.v[S(d.main)->id] >= S(d.main)->pos, "8 hand-over", "the caller is not behind main");
        CHECK(d.sched.sequence_end(d.caller) != 0, "8 hand-over", "sequence_end without a sequence");
        CHECK(d.sched.sequence_begin(d.caller) == 0 && d.sched.sequence_begin(d.caller) != 0, "8 hand-over", "sequence_begin");
        CHECK(is_fenced() == fenced, "8 hand-over", "sequence_begin: fenced = %d in mode %d", (int)is_fenced(), mode);
        int calls = g_records + g_waits;
        CHECK(d.sched.hand_in(d.caller) == 0 && d.sched.hand_out(d.caller) == 0, "8 hand-over", "%s", g_error);
        CHECK(g_records + g_waits == calls, "8 hand-over", "a hand-over inside a sequence on its stream made a runtime call");
        CHECK(d.sched.hand_in(d.other) == 0 && d.sched.hand_out(d.other) == 0, "8 hand-over", "%s", g_error);
        CHECK(g_records + g_waits == calls + 4, "8 hand-over", "another stream's hand-over inside a sequence");
        CHECK(d.sched.sequence_end(d.other) != 0 && d.sched.sequence_end(d.caller) == 0, "8 hand-over", "sequence_end");
        CHECK(S(d.caller)->seen.v[S(d.main)->id] >= S(d.main)->pos, "8 hand-over", "sequence_end: the caller is not behind main");
    }
}

// point 9: a slot whose deferred job is still queued is not handed out
void run_refusal() {
    g_config = "refusal";
    Driver d(Config{});
    const int s = d.claim();
    d.kernel(d.main);
    d.defer(s);
    for (int i = 0; i < NSLOT - 1; ++i) d.claim();
    g_error[0] = 0;
    CHECK(d.sched.next_slot(d.main) != 0 && strstr(g_error, "deferred"), "9 refusal", "slot %d was claimed with its job queued", s);
    CHECK(d.sched.join_side(d.main) == 0 && d.queued == 0, "9 refusal", "%s", g_error);
}
}  // namespace

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i)
        if (!strncmp(argv[i], "--break=", 8)) cdrl_sched_break = atoi(argv[i] + 8);
    int configs = 0;
    for (int lag : {-1, 0, 1, 4, 40})
        for (int tail = 0; tail < 2; ++tail)
            for (int side = 0; side < 2; ++side)
                for (int graph = 0; graph < 2; ++graph) {
                    Config c;
                    c.lag = lag, c.tail = tail, c.side = side, c.graph = graph, c.comm = (configs++ % 3) != 0;
                    run_passes(c);
                }
    run_deferred_errors();
    run_hand_over();
    run_refusal();
    printf("OK %d configurations\n", configs);
    return 0;
}
