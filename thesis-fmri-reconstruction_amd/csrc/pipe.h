// LDS-DMA pipeline pieces shared by the window-resident kernels (igemm_c5.hip, igemm_c5w.hip, igemm_tc5.hip,
// igemm_tc5w.hip, wgrad_win.hip): compile-time loops, buffer descriptors, the buffer -> LDS DMA instruction, counted
// vmcnt waits, the stride-2 tap order, and the MFMA-tile helpers of the two wide kernels' compute waves.  The DMA
// schedules, window address maps and K-steps are the kernels' own.
#pragma once
#include "kernels.h"
#include <type_traits>

namespace fmri {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef uint32_t u4v __attribute__((ext_vector_type(4)));

// f(integral_constant<int, I>) for I in [I, N): loop indices that have to be template / asm-immediate constants
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// raw buffer descriptor over [base, base + bytes): offsets >= bytes read as zero and are not written
__device__ __forceinline__ v4i make_srd(const void* base, uint32_t bytes) {
    return (v4i){(int)(uint32_t)(uintptr_t)base, (int)(uint32_t)((uintptr_t)base >> 32), (int)bytes, 0x00020000};
}

// 16-byte buffer -> LDS DMA: LDS destination = wave-uniform `lds` + lane*16, source = descriptor base + voff + soff.
// Offsets >= num_records read as zero.  Issued from inline asm so that the compiler does not serialise later LDS reads
// behind it (see glds16_raw in common.h); the caller owns the vmcnt / barrier protocol.
__device__ __forceinline__ void bdma16(v4i srd, uint32_t voff, uint32_t soff, uint32_t lds) {
    // under scalar-register pressure the compiler parks the descriptor in vector registers and would hand those to the
    // "s" operand: name every word wave-uniform (free when it already sits in SGPRs)
    srd.x = __builtin_amdgcn_readfirstlane(srd.x);
    srd.y = __builtin_amdgcn_readfirstlane(srd.y);
    srd.z = __builtin_amdgcn_readfirstlane(srd.z);
    srd.w = __builtin_amdgcn_readfirstlane(srd.w);
    soff = __builtin_amdgcn_readfirstlane(soff);
    lds = __builtin_amdgcn_readfirstlane(lds);
    asm volatile("s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, %2 offen lds"
                 ::"v"(voff), "s"(srd), "s"(soff), "s"(lds)
                 : "memory");
}

// ... without a scalar offset: the literal 0 of the instruction (a zero handed over in an SGPR costs an s_mov)
__device__ __forceinline__ void bdma16(v4i srd, uint32_t voff, uint32_t lds) {
    srd.x = __builtin_amdgcn_readfirstlane(srd.x);
    srd.y = __builtin_amdgcn_readfirstlane(srd.y);
    srd.z = __builtin_amdgcn_readfirstlane(srd.z);
    srd.w = __builtin_amdgcn_readfirstlane(srd.w);
    lds = __builtin_amdgcn_readfirstlane(lds);
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(voff), "s"(srd), "s"(lds)
                 : "memory");
}

// at most N vector-memory operations of the wave (DMA pieces and stores, in issue order) stay in flight
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    static_assert(N >= 0 && N <= 63, "vmcnt is a 6-bit field");
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// k5 s2: the 25 taps in phase order: 15 taps of the even rows (ky = 0, 2, 4), then 10 of the odd rows (ky = 1, 3)
constexpr int k5s2_ky(int i) { return i < 15 ? 2 * (i / 5) : 1 + 2 * ((i - 15) / 5); }
constexpr int k5s2_kx(int i) { return i < 15 ? i % 5 : (i - 15) % 5; }

// ---------------------------------------------------------------------------------------------
// the compute waves of the wide kernels (igemm_c5w, igemm_tc5w): wave tile = TN x TM MFMA tiles
// ---------------------------------------------------------------------------------------------
template <int TN, int TM>
__device__ __forceinline__ void zero_acc(f4 (&acc)[TN][TM]) {
#pragma unroll
    for (int i = 0; i < TN; ++i)
#pragma unroll
        for (int j = 0; j < TM; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};
}

// acc += bf x af over all TN x TM tiles.  With the PENDING fragments (the second half of the previous K-step, kept in
// registers across the barrier) these MFMAs cover the fragment reads of the step that has just begun.
template <int TN, int TM>
__device__ __forceinline__ void mfma_tiles(f4 (&acc)[TN][TM], const h8 (&bf)[TN], const h8 (&af)[TM]) {
#pragma unroll
    for (int tn = 0; tn < TN; ++tn)
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
            acc[tn][tm] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[tn], af[tm], acc[tn][tm], 0, 0, 0);
}

// all zeros: nothing pending
template <int N>
__device__ __forceinline__ void clear_frags(h8 (&f)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) f[i] = (h8)(half_t)0.f;
}

// the TM + TN fragment reads issued in front of TM * TN MFMAs go out one by one between the first MFMAs (one read per
// two MFMAs), not as a burst in front of them
template <int TM, int TN>
__device__ __forceinline__ void interleave_reads() {
#pragma unroll
    for (int i = 0; i < TM + TN; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x008, TM * TN - 2 * (TM + TN), 0);
}

}  // namespace fmri
