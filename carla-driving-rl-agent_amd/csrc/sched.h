// Stream scheduler of the learner engine (host code only): its three streams, every event between them and the rules by which they
// are ordered against each other.  The ordering contract, the switches and the measured figures behind each rule: DESIGN.md 3.8;
// tests/host/sched_model.cpp checks the contract on the CPU against a model of the runtime's record / wait semantics.
#pragma once
#include <stdlib.h>

#include <functional>
#include <map>
#include <utility>
#include <vector>

#include "cdrl_host.h"

#ifndef CDRL_SCHED_BROKEN     // defined by the model only: its --break=N disables edge n, to show that its assertions notice
#define CDRL_SCHED_BROKEN(n) false
#endif

namespace cdrl {

class __attribute__((visibility("hidden"))) StreamSched {
public:
    static constexpr int NSLOT = 8;     // rotating scratch sets of the backward's side jobs
    static constexpr int NQ = 3;        // ring of the fused conv backward's partial tiles
    static constexpr int SIDE_HIST = 32;

    StreamSched() = default;
    StreamSched(const StreamSched&) = delete;
    StreamSched& operator=(const StreamSched&) = delete;
    ~StreamSched() {
        for (hipEvent_t e : events_) (void)hipEventDestroy(e);
        for (hipStream_t s : {main_, side_, aux_})
            if (s) (void)hipStreamDestroy(s);
    }

    // streams, events and the switches CDRL_SIDE_STREAM, CDRL_GRAPH, CDRL_DIAG_NOEV, CDRL_EVENT_FENCE, CDRL_SIDE_LAG, CDRL_TAIL_EVENTS
    int create() {
        const char* env = cdrl_getenv("CDRL_SIDE_STREAM");
        side_enabled_ = !(env && atoi(env) == 0);
        const char* genv = cdrl_getenv("CDRL_GRAPH");       // off by default (3.8: replay measured slower than eager launches)
        graphs_enabled_ = genv && atoi(genv) != 0;
        diag_noev_ = cdrl_getenv("CDRL_DIAG_NOEV") ? atoi(cdrl_getenv("CDRL_DIAG_NOEV")) : 0;
        const int prio_lo = 0, prio_hi = 0;                 // all three streams at the default priority (3.8)
        CDRL_HIP(hipStreamCreateWithPriority(&main_, hipStreamNonBlocking, prio_hi));
        CDRL_HIP(hipStreamCreateWithPriority(&side_, hipStreamNonBlocking, prio_lo));
        CDRL_HIP(hipStreamCreateWithPriority(&aux_, hipStreamNonBlocking, prio_lo));
        // Events between the engine's own streams carry no system-scope fence; those that hand over to the communication stream or to a
        // data-parallel caller keep it (3.8).  CDRL_EVENT_FENCE=1 -> default events everywhere.
        const char* fe = cdrl_getenv("CDRL_EVENT_FENCE");
        const unsigned evf_int = hipEventDisableTiming | ((fe && atoi(fe) == 1) ? 0u : (unsigned)hipEventDisableSystemFence);
        for (hipEvent_t* e : {&ev_in_[1], &ev_out_[1], &ev_tail_main_, &ev_tail_side_}) CDRL_TRY(new_event(e, hipEventDisableTiming));
        for (hipEvent_t* e : {&ev_in_[0], &ev_out_[0], &ev_join_, &ev_aux_fork_, &ev_aux_done_}) CDRL_TRY(new_event(e, evf_int));
        for (int i = 0; i < NSLOT; ++i) CDRL_TRY(new_event(&ev_main_[i], evf_int));
        for (int i = 0; i < NSLOT; ++i) CDRL_TRY(new_event(&slots_[i].ev, evf_int));
        for (int i = 0; i < NQ; ++i) CDRL_TRY(new_event(&ring_[i].ev, evf_int));
        for (int i = 0; i < 3; ++i) CDRL_TRY(new_event(&ev_sc_fork_[i], evf_int));
        for (int i = 0; i < 3; ++i) CDRL_TRY(new_event(&ev_sc_done_[i], evf_int));
        // CDRL_SIDE_LAG=-1 -> every claim of a scratch slot waits for its own event; n >= 0: wait_side_record
        const char* le = cdrl_getenv("CDRL_SIDE_LAG");
        side_lag_ = le ? atoi(le) : 4;
        // CDRL_TAIL_EVENTS=0 -> forks by hipEventRecord on the critical stream
        const char* te = cdrl_getenv("CDRL_TAIL_EVENTS");
        tail_.stream = main_;
        if (!(te && atoi(te) == 0) && !graphs_enabled_)
            for (tail_.n = 0; tail_.n < 32; ++tail_.n) CDRL_TRY(new_event(&tail_.ring[tail_.n], evf_int));
        return 0;
    }
    bool created() const { return aux_ != nullptr; }

    hipStream_t main() const { return main_; }      // the critical stream: every public step runs here
    hipStream_t side() const { return side_; }      // filter / bias gradients of the backward, shortcut branches of the forward
    hipStream_t aux() const { return aux_; }        // feature nets + small GRUs (forward and backward)
    bool side_on() const { return side_enabled_; }
    bool graphs() const { return graphs_enabled_; }
    void set_comm(hipStream_t s) { comm_ = s; }
    void note_scaled_pass() { dp_hint_ = true; }    // a pass ran with a gradient scale below 1 (world size > 1)

    // ---- caller hand-over (3.8 point 8): main behind the caller's stream / the caller's stream behind main
    int hand_in(hipStream_t caller) {
        if (!created()) {
            set_error("learner not bound");
            return -1;
        }
        return hand_over(caller, main_, ev_in_);
    }
    int hand_out(hipStream_t caller) { return hand_over(main_, caller, ev_out_); }
    int sequence_begin(hipStream_t caller) {
        if (seq_open_) {
            set_error("sequence_begin: a sequence is already open");
            return -1;
        }
        CDRL_TRY(hand_in(caller));
        seq_open_ = true;
        seq_caller_ = caller;
        return 0;
    }
    int sequence_end(hipStream_t caller) {
        if (!seq_open_ || caller != seq_caller_) {
            set_error("sequence_end: no sequence open on this stream");
            return -1;
        }
        seq_open_ = false;
        return hand_out(caller);
    }

    // ---- eager body of one launch key on main: kernels there carry the stop events learned for this body (TailEvents, cdrl_host.h)
    void begin_body(const std::vector<uint64_t>& key) {
        if (tail_.n == 0) return;
        if (tail_need_.size() > 64) tail_need_.clear();
        std::vector<uint8_t>& need = tail_need_[key];
        if (need.empty()) need.assign(4096, 0);
        tail_.need = need.data();
        tail_.need_cap = (int)need.size();
        tail_.idx = 0;
        tail_.last = nullptr;
        tl_tail = &tail_;
    }
    void end_body() { tl_tail = nullptr; }

    // ---- scratch slots and the ring (point 1): a claim waits for the side job that last read the slot / entry
    int next_slot(hipStream_t st) {
        slot_ = (slot_ + 1) % NSLOT;
        for (const Deferred& d : deferred_)             // its reader is not even enqueued yet: no event could order the claim behind it
            if (d.slot == slot_) {
                set_error("next_slot: a deferred side job of scratch slot %d is still queued", slot_);
                return -1;
            }
        if (diag_noev_ & 1) return 0;
        return wait_side_record(st, slots_[slot_]);
    }
    int slot() const { return slot_; }
    int next_q(hipStream_t st) {
        qi_ = (qi_ + 1) % NQ;
        return wait_side_record(st, ring_[qi_]);
    }
    int q() const { return qi_; }
    // side job that read ring entry qi finished (fused conv backward's reduce): the buffer pair is free again once it has run
    int release_q(int qi, hipStream_t sd) {
        if (!side_enabled_ || sd != side_) return 0;
        return record_side(ring_[qi].ev, &ring_[qi]);
    }

    // ---- forks and joins (points 2, 3, 5, 6)
    // main -> side dependency for the current slot; the deferred jobs go out behind it
    hipStream_t fork_side(hipStream_t st) {
        if (!side_enabled_) return st;
        if (diag_noev_ & 2) return side_;
        if (fork_to(st, side_, ev_main_[slot_]) != 0) return st;
        if (CDRL_SCHED_BROKEN(3)) return side_;
        for (Deferred& d : deferred_) {
            const int rc = d.fn(side_);
            if (rc != 0 && deferred_rc_ == 0) deferred_rc_ = rc;
            // (a job of the current slot is covered by the done_side() that follows)
            if (d.slot != slot_ && record_side(slots_[d.slot].ev, &slots_[d.slot]) != 0 && deferred_rc_ == 0) deferred_rc_ = -3;
        }
        deferred_.clear();
        return side_;
    }
    // side job of the current slot finished
    int done_side(hipStream_t side) {
        if (!side_enabled_ || side != side_) return 0;
        if (deferred_rc_ != 0) return std::exchange(deferred_rc_, 0);
        if ((diag_noev_ & 4) || CDRL_SCHED_BROKEN(2)) return 0;
        return record_side(slots_[slot_].ev, &slots_[slot_]);
    }
    // Side jobs that hang off the main stream but are not urgent (partial reductions of bias / depthwise-filter gradients) are queued
    // and enqueued by the NEXT fork_side (or flush_side / join_side): one event on the critical stream serves several side jobs
    int defer_side(hipStream_t st, std::function<int(hipStream_t)> fn) {
        if (!side_enabled_ || (diag_noev_ & 2)) {
            hipStream_t side = fork_side(st);
            CDRL_TRY(fn(side));
            return done_side(side);
        }
        deferred_.push_back(Deferred{slot_, std::move(fn)});
        return 0;
    }
    // enqueue the deferred side jobs now, behind an event that covers `st`
    int flush_side(hipStream_t st) {
        if (!side_enabled_ || deferred_.empty()) return 0;
        return done_side(fork_side(st));
    }
    // end of a backward: `st` behind the side stream and a pending aux backward, every slot and ring entry free
    int join_side(hipStream_t st) {
        if (!side_enabled_) return 0;
        CDRL_TRY(flush_side(st));
        CDRL_TRY(join_side_at(st, ev_join_));
        if (aux_pending_) CDRL_TRY(join_aux(st));
        for (Claim& c : slots_) c.used = false;
        for (Claim& c : ring_) c.used = false;
        return 0;
    }
    // forward of a stride-2 unit: its shortcut branch runs on the side stream
    int fork_shortcut(hipStream_t st, int stage) { return side_enabled_ ? fork_to(st, side_, ev_sc_fork_[stage]) : 0; }
    int join_shortcut(hipStream_t st, int stage) { return side_enabled_ ? join_side_at(st, ev_sc_done_[stage]) : 0; }
    // the aux stream behind `st`, the end of its work, and who joins it: join_aux in a forward, join_side at the end of a backward
    int fork_aux(hipStream_t st) {
        aux_pending_ = true;
        return fork_to(st, aux_, ev_aux_fork_);
    }
    int done_aux() {
        CDRL_HIP(hipEventRecord(ev_aux_done_, aux_));
        return 0;
    }
    int join_aux(hipStream_t st) {
        if (side_enabled_) CDRL_HIP(hipStreamWaitEvent(st, ev_aux_done_, 0));
        aux_pending_ = false;
        return 0;
    }
    // Point 7, in a backward: the gradients of the heads and of the trunk tail are final once everything enqueued so far has run -- the
    // caller's communication stream is released there.  Under hipGraph capture the external stream must not be pulled into the capture
    // (it would never be joined, and a replay would never release it): the caller falls back to the single post-pass all-reduce.
    int publish_tail(hipStream_t st) {
        if (!comm_ || graphs_enabled_) return 0;
        CDRL_HIP(hipEventRecord(ev_tail_main_, st));          // (recorded, with its system-scope fence: the collectives read these bytes)
        CDRL_HIP(hipStreamWaitEvent(comm_, ev_tail_main_, 0));
        if (!side_enabled_) return 0;
        CDRL_TRY(flush_side(st));       // (queued side jobs go out BEHIND an event of the critical stream, as everywhere else)
        CDRL_HIP(hipEventRecord(ev_tail_side_, side_));
        CDRL_HIP(hipStreamWaitEvent(comm_, ev_tail_side_, 0));
        if (aux_pending_) CDRL_HIP(hipStreamWaitEvent(comm_, ev_aux_done_, 0));
        return 0;
    }

private:
    // a numbered record of the side stream; of a scratch slot or ring entry: the one behind its last side job, if there was one since the last join
    struct Claim { hipEvent_t ev = nullptr; uint64_t seq = 0; bool used = false; };
    struct Deferred { int slot; std::function<int(hipStream_t)> fn; };

    int new_event(hipEvent_t* e, unsigned flags) {
        CDRL_HIP(hipEventCreateWithFlags(e, flags));
        events_.push_back(*e);
        return 0;
    }
    // `to` behind `from`; ev[1] with the system-scope fence for data-parallel use.  Nothing inside a sequence on the sequence's stream.
    int hand_over(hipStream_t from, hipStream_t to, hipEvent_t* ev) {
        if (seq_open_ && (from == seq_caller_ || to == seq_caller_)) return 0;
        hipEvent_t e = ev[comm_ || dp_hint_];
        CDRL_HIP(hipEventRecord(e, from));
        CDRL_HIP(hipStreamWaitEvent(to, e, 0));
        return 0;
    }
    // `to` behind everything `from` holds so far: behind the stop event of its newest kernel when the tail events are on and nothing
    // else went in behind that kernel (nothing is enqueued on `from`), else behind `fallback` recorded on `from`.
    int fork_to(hipStream_t from, hipStream_t to, hipEvent_t fallback) {
        TailEvents* t = tl_tail && from == tl_tail->stream ? tl_tail : nullptr;
        hipEvent_t ev = t ? t->last : nullptr;
        if (!ev) {
            if (t && t->idx > 0 && t->idx <= t->need_cap) t->need[t->idx - 1] = 1;     // next run: a stop event on that launch
            CDRL_HIP(hipEventRecord(fallback, from));
            ev = fallback;
        }
        CDRL_HIP(hipStreamWaitEvent(to, ev, 0));
        return 0;
    }
    // record `ev` on the side stream and number the record; c: the scratch slot or ring entry that is free once it is covered
    int record_side(hipEvent_t ev, Claim* c = nullptr) {
        CDRL_HIP(hipEventRecord(ev, side_));
        ++side_seq_;
        side_hist_[side_seq_ % SIDE_HIST] = Claim{ev, side_seq_};
        if (c) c->seq = side_seq_, c->used = true;
        return 0;
    }
    // `st` joins the side stream: `ev` recorded there (numbered) and waited for; the critical stream has then waited for that record
    int join_side_at(hipStream_t st, hipEvent_t ev) {
        CDRL_TRY(record_side(ev));
        CDRL_HIP(hipStreamWaitEvent(st, ev, 0));
        if (st == main_) main_waited_ = side_seq_;
        return 0;
    }
    // The lagged wait (3.8 point 4): records on the side stream are numbered, the critical stream remembers the newest one it waited for
    int wait_side_record(hipStream_t st, const Claim& c) {
        if (!side_enabled_ || !c.used || CDRL_SCHED_BROKEN(1)) return 0;
        if (st != main_ || side_lag_ < 0) {              // another stream than the critical one (or the scheme off): the claim's own event
            CDRL_HIP(hipStreamWaitEvent(st, c.ev, 0));
            return 0;
        }
        if (c.seq <= main_waited_) return 0;
        uint64_t target = c.seq;
        if (side_seq_ > (uint64_t)side_lag_ && side_seq_ - (uint64_t)side_lag_ > target) target = side_seq_ - (uint64_t)side_lag_;
        hipEvent_t ev = c.ev;
        uint64_t covered = c.seq;
        if (side_seq_ - target < SIDE_HIST && side_hist_[target % SIDE_HIST].seq == target) {
            ev = side_hist_[target % SIDE_HIST].ev;
            covered = target;
        }
        for (int i = 0; i < SIDE_HIST; ++i)             // the event may have been recorded again since: waiting for it covers that record too
            if (side_hist_[i].ev == ev && side_hist_[i].seq > covered) covered = side_hist_[i].seq;
        CDRL_HIP(hipStreamWaitEvent(st, ev, 0));
        main_waited_ = covered;
        return 0;
    }

    hipStream_t main_ = nullptr, side_ = nullptr, aux_ = nullptr, comm_ = nullptr;
    std::vector<hipEvent_t> events_;                     // every event create() made
    bool side_enabled_ = true, graphs_enabled_ = true;
    int diag_noev_ = 0;                                  // CDRL_DIAG_NOEV: timing diagnostics only (racy)
    hipEvent_t ev_in_[2] = {}, ev_out_[2] = {};          // hand-over: [0] within the device, [1] with the system-scope fence
    bool dp_hint_ = false, seq_open_ = false;
    hipStream_t seq_caller_ = nullptr;
    TailEvents tail_;
    std::map<std::vector<uint64_t>, std::vector<uint8_t>> tail_need_;      // per body (launch key): which launches a fork follows
    hipEvent_t ev_main_[NSLOT] = {}, ev_join_ = nullptr, ev_sc_fork_[3] = {}, ev_sc_done_[3] = {};
    hipEvent_t ev_aux_fork_ = nullptr, ev_aux_done_ = nullptr, ev_tail_main_ = nullptr, ev_tail_side_ = nullptr;
    Claim slots_[NSLOT], ring_[NQ];
    int slot_ = 0, qi_ = 0, side_lag_ = 4;
    Claim side_hist_[SIDE_HIST];                         // the newest records of the side stream ...
    uint64_t side_seq_ = 0, main_waited_ = 0;            // ... and the newest one the critical stream has waited for
    std::vector<Deferred> deferred_;
    int deferred_rc_ = 0;
    bool aux_pending_ = false;
};

}  // namespace cdrl
