// unit_common.h -- the host pieces every front-end unit (triangulate.hip ... cloud_merge.hip) shares: what a unit returns to its
// wrapper in api_frontend.hip, the early-return macros, and the per-phase HIP-event timer.  Nothing here is part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstdlib>
#include <vector>

namespace sfmba {

// What a unit returns besides 0 (ok) and positive hipError_t codes; api_frontend.hip maps them to SFMBA_ERR_* and a message.
enum {
    UNIT_ERR_CAPACITY = -1,        // the outputs are too small; *total holds the size that is needed
    UNIT_ERR_TOO_LARGE = -2,       // a count of the call does not fit the unit's indices (the wrapper names the limit)
    UNIT_ERR_SIZE = -3,            // the resize factor gives an image a side outside 1..16384 (nothing was written)
    UNIT_ERR_HOST_ALLOC = -4,      // no host memory
};

// a hipError_t that is not hipSuccess ends the unit's call
#define UNIT_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)
#define UNIT_ALLOC(arena, ptr, T, n) do { ptr = (arena).alloc_n<T>(n); if (!ptr) return (int)hipErrorOutOfMemory; } while (0)
// the same for the image readers, whose per-group arena and host tables go out of scope with the return: the stream `s` of the
// enclosing function is drained first, so that nothing queued may still use them
#define UNIT_DRAIN_TRY(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { (void)hipStreamSynchronize(s); return (int)e_; } } while (0)
#define UNIT_DRAIN_ALLOC(arena, ptr, T, n) \
    do { ptr = (arena).alloc_n<T>(n); if (!ptr) { (void)hipStreamSynchronize(s); return (int)hipErrorOutOfMemory; } } while (0)

// The limits of a group of the units that take their images, jobs or pairs in consecutive groups (orb_extract.hip ... flow_track.hip).
// SFMBA_GROUP_BYTES and SFMBA_GROUP_ITEMS are test hooks that lower the unit's scratch budget and its cap on the items of a group, so
// that the multi-group path runs at test size; read once per call.  Only a positive decimal integer below the unit's constant
// counts: anything else (absent, empty, zero, negative, not a number, trailing text) leaves the constant, so a limit is never
// raised.  The first item of a group enters it whatever the limits say.
inline long long group_limit_from(const char* text, long long unit_limit) {
    if (!text || !*text) return unit_limit;
    char* end = nullptr;
    errno = 0;
    const long long v = std::strtoll(text, &end, 10);
    if (errno != 0 || end == text || *end != '\0' || v <= 0) return unit_limit;
    return v < unit_limit ? v : unit_limit;
}
inline long long group_bytes_limit(size_t unit_bytes) { return group_limit_from(std::getenv("SFMBA_GROUP_BYTES"), (long long)unit_bytes); }
inline int group_items_limit(int unit_items) { return (int)group_limit_from(std::getenv("SFMBA_GROUP_ITEMS"), unit_items); }

// HIP-event time per phase, summed; inert without a timing array.  begin / end bracket one phase; next ends the open phase and
// begins another on the same event, so consecutive phases leave no gap.
struct PhaseTimer {
    struct Span { int phase, first, last; };
    hipStream_t s;
    bool on;
    std::vector<hipEvent_t> ev;
    std::vector<Span> span;
    void begin(int p) { if (on) span.push_back(Span{ p, mark(), -1 }); }
    void end() { if (on) span.back().last = mark(); }
    void next(int p) { if (on) { const int e = mark(); span.back().last = e; span.push_back(Span{ p, e, -1 }); } }
    int mark() { hipEvent_t e = nullptr; if (hipEventCreate(&e) == hipSuccess) (void)hipEventRecord(e, s); ev.push_back(e); return (int)ev.size() - 1; }
    void collect(double* t) {
        for (const Span& p : span) {
            float ms = 0.f;
            if (p.last >= 0 && ev[p.first] && ev[p.last] && hipEventElapsedTime(&ms, ev[p.first], ev[p.last]) == hipSuccess) t[p.phase] += ms;
        }
    }
    ~PhaseTimer() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};

}  // namespace sfmba
