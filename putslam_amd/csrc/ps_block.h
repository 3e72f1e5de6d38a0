// ps_block.h -- the work-group and wave primitives of the kernel headers, once: ordered compaction (flag scans), the integer
// scan, the maximum, wave minima, the lock-free union-find, the XCD-aware work-group order, the phase stamp and the wave-uniform
// mask helpers.  Nothing here knows a kernel; every LDS scratch block is the caller's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ps_device_math.h" // PS_D

namespace psdev {

constexpr int kBlock = 256;

// ---- ordered compaction ----
// The exclusive prefix of `flag` over the BLOCK threads of the work-group, in thread order; `total` = number of set flags.
// TRAIL: a second barrier follows the reads of the wave sums, so `wsum2` (BLOCK / 64 ints) may be written again at once.
// !TRAIL: ONE barrier per call.  `wsum2` then holds two sets of BLOCK / 64 slots and `parity` (the call's number, uniform over
// the work-group) picks one.  A slot is written again two calls later, behind the barrier of the call in between, which every
// thread reaches only after it has read the slot.
template <int BLOCK = kBlock, bool TRAIL = true>
__device__ __forceinline__ int block_scan_flag(bool flag, int &total, int *wsum2, int parity = 0)
{
    int *wsum = wsum2 + (parity & 1) * (BLOCK / 64);
    unsigned long long bal = __ballot(flag);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int pre = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < BLOCK / 64; ++i) {
        int s = wsum[i];
        if (i < w) off += s;
        total += s;
    }
    if (TRAIL) __syncthreads();
    return off + pre;
}

// Two ordered compactions with the barriers of one: exclusive prefixes of flagA and flagB over the work-group (flagB implies
// nothing about flagA); the wave sums travel packed (A in the low 16 bits, B in the high ones).  TRAIL / parity as above.
template <int BLOCK = kBlock, bool TRAIL = true>
__device__ __forceinline__ void block_scan_flags2(bool flagA, bool flagB, int &posA, int &totalA, int &posB, int &totalB,
                                                  int *wsum2, int parity = 0)
{
    int *wsum = wsum2 + (parity & 1) * (BLOCK / 64);
    const unsigned long long ba = __ballot(flagA), bb = __ballot(flagB);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    if (lane == 0) wsum[w] = __popcll(ba) | (__popcll(bb) << 16);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < BLOCK / 64; ++i) {
        const int sv = wsum[i];
        if (i < w) off += sv;
        tot += sv;
    }
    if (TRAIL) __syncthreads();
    posA = (off & 0xFFFF) + __popcll(ba & below);
    posB = (off >> 16) + __popcll(bb & below);
    totalA = tot & 0xFFFF;
    totalB = tot >> 16;
}

// exclusive prefix of v over the work-group, in thread order; total = the sum
template <int BLOCK> __device__ __forceinline__ int block_scan_int(int v, int &total, int *wsum)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int off = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < BLOCK / 64; ++i) {
        const int s = wsum[i];
        if (i < w) off += s;
        total += s;
    }
    __syncthreads();
    return off + incl - v;
}

// ---- maximum ----
// workgroup-wide maxima of two non-negative floats with one pair of barriers
template <int BLOCK = kBlock> __device__ __forceinline__ void block_max2(float &a, float &b, float2 *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a = fmaxf(a, __shfl_down(a, o, 64));
        b = fmaxf(b, __shfl_down(b, o, 64));
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = make_float2(a, b);
    __syncthreads();
    float2 r = red[0];
#pragma unroll
    for (int i = 1; i < BLOCK / 64; ++i) {
        r.x = fmaxf(r.x, red[i].x);
        r.y = fmaxf(r.y, red[i].y);
    }
    __syncthreads();
    a = r.x;
    b = r.y;
}

// ---- wave minima, the result in every lane ----
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unsigned long long other = __shfl_down(v, o, 64);
        v = other < v ? other : v;
    }
    return __shfl(v, 0, 64);
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_down((int)v, o, 64);
        v = other < v ? other : v;
    }
    return (uint32_t)__shfl((int)v, 0, 64);
}

// ---- lock-free union-find ----
// par[] is shared by the threads of one work-group (SCOPE = __HIP_MEMORY_SCOPE_WORKGROUP: DBScan's, in LDS) or by the
// work-groups of a launch (__HIP_MEMORY_SCOPE_AGENT: the exclusion filters', in global memory).  Every root is the least
// index of its tree: a root is only ever hooked under a smaller one.
template <int SCOPE> __device__ __forceinline__ int uf_find(int *par, int x)
{
    int p = __hip_atomic_load(&par[x], __ATOMIC_RELAXED, SCOPE);
    while (p != x) {
        const int g = __hip_atomic_load(&par[p], __ATOMIC_RELAXED, SCOPE);
        if (g != p) __hip_atomic_store(&par[x], g, __ATOMIC_RELAXED, SCOPE); // path halving
        x = p;
        p = g;
    }
    return x;
}

template <int SCOPE> __device__ __forceinline__ void uf_union(int *par, int a, int b)
{
    for (;;) {
        a = uf_find<SCOPE>(par, a);
        b = uf_find<SCOPE>(par, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicCAS(&par[b], b, a);
        if (old == b) return;
        b = old; // b was hooked meanwhile: retry from where it went
    }
}

// ---- work-group order, phase stamps ----
// XCD-aware work-group order.  Work-groups are dealt round-robin over the 8 XCDs (each with its own
// 4 MiB L2), so linear ids L and L+8 share an L2.  This bijection gives every XCD a CONTIGUOUS range of
// logical ids, so the work-groups that sweep the same frame pair (same query rows / same match records)
// run on one XCD and re-read them from its L2 instead of each XCD fetching its own copy.  Speed only:
// nothing depends on where a work-group actually lands.
PS_D unsigned xcd_remap(unsigned L, unsigned total)
{
    const unsigned xcd = L & 7u, idx = L >> 3;
    const unsigned q = total >> 3, r = total & 7u;
    return (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + idx;
}

// Phase stamps of the latency study (option "stamps", ps_debug_stamps): thread 0 of work-group 0 writes the shader clock
// (s_memtime) at the phase boundaries of kernels 2 and 4 into a private buffer -- never into outputs.  stamps == nullptr in
// every ordinary launch (one scalar compare per boundary).
PS_D void phase_stamp(unsigned long long *stamps, int i)
{
    if (stamps != nullptr && threadIdx.x == 0 && blockIdx.x == 0) stamps[i] = __builtin_readcyclecounter();
}

// ---- wave-uniform masks ----
// wave-uniform "every active lane satisfies p": compares the ballot with the exec mask directly, so the
// predicate never has to be materialised in a VGPR (hipcc's __all() costs a v_cndmask + v_cmp_ne)
PS_D bool wave_all(bool p) { return __builtin_amdgcn_ballot_w64(p) == __builtin_amdgcn_ballot_w64(true); }

// Lanes of a wave-uniform 64-bit mask without lane masks in vector registers ((1 << lane) - 1 and its complement are four
// registers the compiler hoists out of every loop): how many set bits lie below the calling lane (v_mbcnt_lo / _hi),
// and whether the calling lane's own bit is set (v_cndmask with the mask as the selector).
PS_D int lanes_below(unsigned long long mask)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
// a 64-bit value that is the same in every lane, moved to scalar registers (loaded through a pointer the compiler cannot
// prove uniform it sits in vector registers)
PS_D unsigned long long uniform64(unsigned long long v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}
PS_D bool lane_in(unsigned long long mask)
{
    int x;
    asm("v_cndmask_b32 %0, 0, 1, %1" : "=v"(x) : "s"(mask));
    return x != 0;
}
// cnt += 1 in the lanes of `mask` (v_addc_co_u32 with the mask as carry-in: one VALU op)
PS_D void add_mask(int &cnt, unsigned long long mask)
{
    asm volatile("v_addc_co_u32 %0, vcc, 0, %0, %1" : "+v"(cnt) : "s"(mask) : "vcc");
}

} // namespace psdev
