// Host-only helpers of libcdrl_hip.so: error reporting, the CDRL_* switches and the tail-event bookkeeping.  No device code: this
// header compiles as plain C++ (the stream scheduler's host model, tests/host/sched_model.cpp, includes it through sched.h).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace cdrl {

void set_error(const char* fmt, ...);
const char* last_error();
// getenv for the library's CDRL_* switches: CDRL_DIAG_* (wrong-result timing diagnostics) only with the master CDRL_DIAG=1
const char* cdrl_getenv(const char* name);

#define CDRL_HIP(expr)                                                                         \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            cdrl::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); \
            return -2;                                                                         \
        }                                                                                      \
    } while (0)

#define CDRL_TRY(expr)            \
    do {                          \
        int _r = (expr);          \
        if (_r != 0) return _r;   \
    } while (0)

// Tail events (round 6): a fork to another stream used to be hipEventRecord on the critical stream -- a barrier packet of its own in
// the queue, a bubble in front of the next kernel, ~70 times per update-step.  hipExtLaunchKernelGGL binds a STOP EVENT to the kernel's
// own dispatch packet instead (its completion signal), so the other stream can wait for "the newest kernel of the critical stream"
// without anything being enqueued there.  A stop event on EVERY kernel costs more than the bubbles it removes (+0.16 ms per
// update-step), so the launches that need one are LEARNED: while a thread has a TailEvents installed (StreamSched::begin_body), launch
// number i of the body carries an event iff a fork followed launch i the last time this body ran (`need`); a fork that finds no event
// behind the newest kernel (`last` null: first run, a changed sequence, a copy or memset behind the kernel) records one the old way and
// marks the launch for the next run.  Always correct; converges after one run of each body.
struct TailEvents {
    hipStream_t stream = nullptr;
    hipEvent_t ring[32] = {};
    int n = 0;
    unsigned head = 0;
    hipEvent_t last = nullptr;      // stop event of the newest kernel on `stream`, if it carries one
    int idx = 0;                    // launches of this body on `stream` so far
    uint8_t* need = nullptr;        // per launch index of the current body: 1 = a fork followed it
    int need_cap = 0;
};
extern thread_local TailEvents* tl_tail;

// One kernel launch on `st` (launch_tracked, cdrl_common.h): the stop event it has to carry, or null for a plain launch
inline hipEvent_t tail_note_launch(hipStream_t st) {
    TailEvents* t = tl_tail;
    if (t && st == t->stream) {
        const int i = t->idx++;
        if (i < t->need_cap && t->need[i]) return t->last = t->ring[t->head++ % (unsigned)t->n];
        t->last = nullptr;
    }
    return nullptr;
}
// something that is not a kernel (a copy, a memset) went onto `st` behind its newest kernel
inline void tail_invalidate(hipStream_t st) {
    TailEvents* t = tl_tail;
    if (t && st == t->stream) t->last = nullptr;
}

}  // namespace cdrl
