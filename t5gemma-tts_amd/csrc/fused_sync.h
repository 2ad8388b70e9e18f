// Hand-off primitives of the persistent decode launches (fused_kernels.h): the counter-set
// layout, the bounded poll, the barriers and the publish.
//
// Hand-offs (gfx950 recipe, cdna_hip_programming.md Guideline 16 R1): the handed-off
// bytes (xn rows, act) are stored write-through (sc1) by every storing wave, each storing
// wave drains (vmcnt(0)), the workgroup meets at a barrier, ONE lane adds to a relaxed
// agent-scope counter (one per 128-byte line); the consumer polls that counter relaxed from
// ONE wave (which has no weight loads queued ahead of the poll), the workgroup meets at a
// barrier, and every load of the handed-off bytes is an sc1 load. Counter sets start at
// zero (zeroed at engine creation and by the host after a timeout); each decoder layer has
// its own set, and each launch zeroes the NEXT layer's set as it starts (that set's last
// user has completed), so no arrival count is needed at the end. Every wait is bounded:
// a wait that gives up stores a
// timeout code that makes every later wait give up at once (outputs are then garbage and
// the host raises, t5g_read_tokens); no wave can spin forever.
#pragma once
#include "common.h"
#include "t5g_kernels.h"

namespace t5g {

constexpr int FM_NW = 12;         // waves per workgroup (the gate/up and down kernels' count)
constexpr int FM_NS = 4;          // cross-o split-K slabs read by the norm stage
constexpr int FM_DS = 8;          // down-projection k-slices
constexpr int FM_NORM_UNITS = 3;  // gate/up units of a norm workgroup (tools/diag_fused.py)
constexpr unsigned FM_SPIN_MAX = 1u << 18;   // ~0.3-0.5 s of polling before a wait gives up

// lines of a counter set (FusedMlpArgs::sync), one word per 128-byte line
constexpr int L_N1 = 0, L_Q0 = 1, L_A0 = 9, L_O0 = 17, L_N2 = 25, L_SL0 = 26, L_D0 = 34, L_N3 = 42, L_P0 = 43,
              L_S0 = 51, L_K0 = 59;
static_assert(L_K0 + 8 == FM_SET_LINES, "counter set layout");
__device__ __forceinline__ unsigned* cline(unsigned* set, int line) { return set + line * FM_LINE; }
constexpr int FS_NORM = L_N2 * FM_LINE;
__device__ __forceinline__ int fs_slice(int s) { return (L_SL0 + s) * FM_LINE; }

__device__ __forceinline__ unsigned ld_rlx(unsigned* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one wave polls N counter lines of a set at once (lane i reads line line0 + i, lane 63 the
// timeout word): every round is ONE memory round trip whatever N is; true when every line
// has reached its target, false on a timeout (this wait's or an earlier one's). SPLIT: the N
// lines share `target` arrivals round-robin (arrival k goes to line k % N), so line i waits
// for (target - i + N - 1) / N.
template <int N, bool SPLIT = false>
__device__ __forceinline__ bool fm_wait_n(unsigned* set, int line0, unsigned target, unsigned* tmo, unsigned code) {
    static_assert(N >= 1 && N < 64, "lines per poll");
    const int lane = threadIdx.x & 63;
    const int li = min(lane, N - 1);
    unsigned* p = lane == 63 ? tmo : set + (line0 + li) * FM_LINE;
    if constexpr (SPLIT) target = (target + (unsigned)(N - 1 - li)) / (unsigned)N;
    for (unsigned spins = 0;; ++spins) {
        const unsigned v = ld_rlx(p);
        if (__all(lane == 63 || v >= target)) return true;
        if (__shfl(v, 63, 64) != 0) return false;
        if (spins > FM_SPIN_MAX) {
            if (lane == 0) __hip_atomic_store(tmo, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return false;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}
template <int N>
__device__ __forceinline__ bool fm_wait_split(unsigned* set, int line0, unsigned total, unsigned* tmo, unsigned code) {
    return fm_wait_n<N, true>(set, line0, total, tmo, code);
}

// workgroup rendezvous with no memory semantics for the compiler to add waits for (the
// weight loads in flight must stay in flight across it); the "memory" clobber keeps the
// handed-off loads below it
__device__ __forceinline__ void wg_barrier() { asm volatile("s_barrier" ::: "memory"); }
__device__ __forceinline__ void drain_vm() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

__device__ __forceinline__ __amdgpu_buffer_rsrc_t raw_rsrc(const void* base, uint32_t bytes) {
    const uint64_t p = (uint64_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
    return __builtin_amdgcn_make_buffer_rsrc((void*)(((uint64_t)hi << 32) | lo), 0,
                                             (int)__builtin_amdgcn_readfirstlane(bytes), 0x00020000);
}
constexpr int AUX_NT = 2, AUX_SC1 = 16;

// barrier that waits for this wave's LDS traffic only (no vmcnt: loads stay in flight)
__device__ __forceinline__ void fb_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// every storing wave drains, the workgroup meets, one lane adds `n` to `ctr`
__device__ __forceinline__ void fb_publish(unsigned* ctr, unsigned n) {
    drain_vm();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_fetch_add(ctr, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace t5g
