// rs_host.h -- host plumbing the handles share (rs_handle, kb_handle and what hangs off them): the error convention, the
// event pairs of the kernel timing, stream-to-stream edges and the hash of the checkpoints.  Host only: no device code.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/ranslice.h"

// a failed HIP call leaves its text in the handle's `err` and returns RS_EHIP from the calling function
#define HIPCHK(h, call)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            (h)->err = std::string(#call) + ": " + hipGetErrorString(e_);                            \
            return RS_EHIP;                                                                          \
        }                                                                                            \
    } while (0)

// ---- kernel timing: a growing pool of event pairs, each around one launch (or one phase) on a stream and tagged with a kind.
// The caller records the second event of a pair itself, after the launches it wants bracketed.
struct EventSpans {
    struct Span {
        hipEvent_t e0, e1;
        int kind;
    };
    bool on = false;
    std::vector<Span> spans;
    size_t used = 0;

    // *end = the event to record behind the launches; nullptr (and nothing recorded, the pool untouched) while timing is off
    hipError_t begin(hipStream_t stream, int kind, hipEvent_t* end) {
        *end = nullptr;
        if (!on) return hipSuccess;
        if (used == spans.size()) {
            Span s = {nullptr, nullptr, 0};
            for (hipEvent_t* ev : {&s.e0, &s.e1}) {
                const hipError_t e = hipEventCreate(ev);
                if (e != hipSuccess) return e;
            }
            spans.push_back(s);
        }
        Span& s = spans[used];
        s.kind = kind;
        const hipError_t e = hipEventRecord(s.e0, stream);
        if (e != hipSuccess) return e;
        *end = s.e1;
        used++;
        return hipSuccess;
    }
    // fn(kind, ms) for every pair taken since the last drain or reset, in the order taken (the stream must have been waited for)
    template <class F>
    hipError_t drain(F fn) {
        for (size_t i = 0; i < used; ++i) {
            float ms = 0.f;
            const hipError_t e = hipEventElapsedTime(&ms, spans[i].e0, spans[i].e1);
            if (e != hipSuccess) return e;
            fn(spans[i].kind, (double)ms);
        }
        used = 0;
        return hipSuccess;
    }
    void reset() { used = 0; }
    void release() {
        for (Span& s : spans) {
            (void)hipEventDestroy(s.e0);
            (void)hipEventDestroy(s.e1);
        }
        spans.clear();
        used = 0;
    }
};

// ---- stream edges.  The events are made on first use, without timing.
template <class H>
static int ensure_event(H* h, hipEvent_t* e) {
    if (!*e) HIPCHK(h, hipEventCreateWithFlags(e, hipEventDisableTiming));
    return RS_OK;
}

// what is enqueued on `to` from here on runs after what is queued on `from` now
template <class H>
static int stream_after(H* h, hipEvent_t* e, hipStream_t from, hipStream_t to) {
    const int rc = ensure_event(h, e);
    if (rc != RS_OK) return rc;
    HIPCHK(h, hipEventRecord(*e, from));
    HIPCHK(h, hipStreamWaitEvent(to, *e, 0));
    return RS_OK;
}

// ---- FNV-1a, 64 bit: the hash of the checkpoint headers and of what two handles must share to fork between them.
// fnv1a_step folds one value in (a byte, or a whole 64-bit word as the region sizes are); fnv1a folds a run of bytes.
static const uint64_t kFnvOffsetBasis = 1469598103934665603ull;
static inline uint64_t fnv1a_step(uint64_t h, uint64_t v) { return (h ^ v) * 1099511628211ull; }
static inline uint64_t fnv1a(const void* p, size_t n, uint64_t h = kFnvOffsetBasis) {
    const unsigned char* c = (const unsigned char*)p;
    for (size_t i = 0; i < n; ++i) h = fnv1a_step(h, c[i]);
    return h;
}
