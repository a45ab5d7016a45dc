// rt_handout.h — how the waves of a persistent kernel (k_wf_mesh, k_wf_intersect) share a queue of n entries.
//
// W waves serve the queue.  Wave g starts on the static range [g*s0, (g+1)*s0) without touching memory; the shared cursor
// (WfCounters::cursor, counts from 0) then serves the entries from W*s0 on, in ranges of 256 entries while much of the queue
// is left and of 128 and 64 towards its end, so that the last waves of a launch finish a short range each instead of one
// wave working through 256 entries alone.  A wave sizes its next reservation from what it already holds - n, W and the end
// of its own last range, which is a lower bound of the cursor - so a reservation is still ONE atomic and no extra round trip.
//
// Written once, __host__ __device__: the kernels call handout_next with the wave's atomic, rt_debug_handout_replay (tests
// without a GPU) with a plain counter.
//
// Atomics per launch: the cursor is touched only when n > W*s0, i.e. n > 256 W, and then serves n - 256 W entries.  Ranges
// of 128 are made only while fewer than left256 * W entries are left behind the asking wave's last range (hence behind the
// cursor), ranges of 64 while fewer than left128 * W are; every wave makes one last atomic that finds the queue empty,
// except the wave whose range ended at n.  With left256 + 2 * left128 <= 768 that is at most n/256 + 4 W
// (tests/test_handout_host.py counts them).
#pragma once
#include <cstdint>

#if defined(__HIP__)
#include <hip/hip_runtime.h>
#define RT_HANDOUT_HD __host__ __device__ __forceinline__
#else
#define RT_HANDOUT_HD inline
#endif

namespace rt {

constexpr uint32_t kHandoutMax = 256;  // largest range (= WF_BATCH), and the staging area of a wave of k_wf_mesh<double>
constexpr uint32_t kHandoutMin = 64;   // smallest range, except the one that ends at n

// Kernel argument.  mode 0: no static range, every reservation 256 entries (the hand-out before this policy: A/B control);
// 1: static first range + shrinking ranges; 2: 1 + the range's entries staged in LDS (k_wf_mesh).
struct HandoutPolicy {
    uint32_t mode;
    uint32_t left256;  // ranges of 256 while at least this many entries PER WAVE are left, ...
    uint32_t left128;  // ... of 128 while at least this many are, of 64 below
};
// A wave's own last range lags the cursor by about one round of the other waves' reservations (W * 256, then W * 128
// entries), so these thresholds shrink the ranges when about 128 and 64 entries per wave are really left.
// Sweep: profiles/mesh_handout/threshold_sweep.txt
constexpr uint32_t kHandoutLeft256 = 384, kHandoutLeft128 = 192;

// s0: ceil(n / W) rounded up to a multiple of 64, inside 64..256 (0: no static range)
RT_HANDOUT_HD uint32_t handout_first(HandoutPolicy hp, uint32_t n, uint32_t W) {
    if (hp.mode == 0u) return 0u;
    const uint64_t per = (uint64_t(n) + W - 1u) / W;
    const uint64_t s = (per + 63u) & ~uint64_t(63);
    return s < kHandoutMin ? kHandoutMin : (s > kHandoutMax ? kHandoutMax : uint32_t(s));
}

// The static range of wave g: [*cur, *end), empty when it starts at or behind n.
RT_HANDOUT_HD void handout_static(uint32_t n, uint32_t s0, uint32_t g, uint32_t* cur, uint32_t* end) {
    const uint64_t a = uint64_t(g) * s0, b = a + s0;
    *cur = a < n ? uint32_t(a) : n;
    *end = b < n ? uint32_t(b) : n;
}

// Size of the reservation of a wave whose last range ended at `pos` (>= W*s0).
RT_HANDOUT_HD uint32_t handout_size(HandoutPolicy hp, uint32_t n, uint32_t W, uint32_t pos) {
    if (hp.mode == 0u) return kHandoutMax;
    const uint64_t left = n > pos ? n - pos : 0u;
    if (left >= uint64_t(hp.left256) * W) return 256u;
    if (left >= uint64_t(hp.left128) * W) return 128u;
    return 64u;
}

// What a wave does when its range [.., last_end) is used up: reserves the next one, [*base, *end), through
// `add(size)` (= atomicAdd on the cursor, returns the old value), or learns that the queue has been handed out (false).
template <typename Add>
RT_HANDOUT_HD bool handout_next(HandoutPolicy hp, uint32_t n, uint32_t W, uint32_t start, uint32_t last_end, Add&& add,
                                       uint32_t* base, uint32_t* end) {
    // start = W * s0: the cursor serves the entries from there on (W <= 2^16 waves: no overflow)
    if (hp.mode != 0u && (start >= n || last_end >= n)) return false;  // the static ranges cover the queue / this wave held its end
    const uint32_t size = handout_size(hp, n, W, last_end > start ? last_end : start);
    const uint32_t b = start + add(size);
    if (b >= n) return false;
    *base = b;
    *end = n - b < size ? n : b + size;
    return true;
}

}  // namespace rt
