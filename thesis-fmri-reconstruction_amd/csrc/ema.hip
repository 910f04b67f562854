// Exponential moving average of the weights (include/fmri_hip.h fmri_ema_update for the semantics; fmri_hip/ema.py).
//
//   ema_kernel<0>   shadow <- shadow + (1 - d) * (live - shadow) over every segment of a table, one launch.  d is derived by
//                   every block from the same 16-byte fmri_ema_state block, which nothing in the launch writes.
//   ema_kernel<1>   live <-> shadow, as 32-bit words (NaN payloads survive), over the same tables.
//
// Both are streaming kernels in the mould of state_copy_kernel (csrc/state.hip): a chunk (FMRI_EMA_CHUNK floats of one
// segment) is one block's unit of work; blocks walk the chunks grid-stride and find a chunk's segment by binary search over
// the table's running chunk counts; 16 bytes per lane and access, every load of a chunk issued in front of its first store,
// a dword tail, and a dword-by-dword path for a segment whose two bases are not both 16-byte aligned.  No byte outside
// [base, base + 4 n) of either side is touched.
#include "../../include/fmri_hip.h"
#include "common.h"
#include "kernels.h"

namespace fmri {

namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int VEC_PER_LANE = FMRI_EMA_CHUNK / (THREADS * 4);         // 16-byte accesses per lane, side and chunk
static_assert(VEC_PER_LANE * THREADS * 4 == FMRI_EMA_CHUNK, "a chunk is a whole number of 16-byte accesses per lane");

// The decay of step t -- the ONE expression the kernel, fmri_ema_decay_at and with it the tests' oracle share.  The
// warm-up quotient is taken in double (as the schedules of csrc/schedule.hip are) and rounded to fp32 once.
__host__ __device__ inline float decay_at(int32_t t, int32_t start, float decay, int32_t warmup) {
    if (t < start) return 0.f;                                        // copy: e + 1 * (w - e)
    if (!warmup) return decay;
    const double s = (double)t - (double)start;
    const float w = (float)((1.0 + s) / (10.0 + s));
    return w < decay ? w : decay;
}

// fp32, in exactly this order (the library is built with -ffp-contract=off: no fused multiply-add)
__device__ __forceinline__ float ema1(float e, float w, float omd) { return e + omd * (w - e); }

// OP 0: update the shadows, OP 1: exchange live and shadow
template <int OP>
__global__ __launch_bounds__(THREADS) void ema_kernel(const fmri_ema_seg* __restrict__ segs, int nseg, int64_t chunks,
                                                      const fmri_ema_state* __restrict__ state) {
    float omd = 0.f;
    if (OP == 0) omd = 1.0f - decay_at(state->t, state->start, state->decay, state->warmup);
    const int tid = threadIdx.x;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        // the last segment whose first chunk is <= c (empty segments share their successor's chunk0 and sort in front)
        int lo = 0, hi = nseg - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (segs[mid].chunk0 <= c) lo = mid;
            else hi = mid - 1;
        }
        const fmri_ema_seg s = segs[lo];
        const int64_t f0 = (c - s.chunk0) * FMRI_EMA_CHUNK;           // < s.n: c is one of the segment's chunks
        const int n = (int)(s.n - f0 < FMRI_EMA_CHUNK ? s.n - f0 : FMRI_EMA_CHUNK);
        float* const live = s.live + f0;
        float* const shadow = s.shadow + f0;
        if ((((uintptr_t)s.live | (uintptr_t)s.shadow) & 15) == 0) {
            // both sides 16-byte aligned (a chunk is a multiple of 16 bytes): 16 bytes per lane, every load of the chunk
            // issued in front of the first store
            const int nv = n >> 2;
            u4 w[VEC_PER_LANE], e[VEC_PER_LANE];
#pragma unroll
            for (int k = 0; k < VEC_PER_LANE; ++k) {
                const int i = tid + k * THREADS;
                w[k] = e[k] = (u4)(0u);
                if (i < nv) {
                    w[k] = *((const u4*)live + i);
                    e[k] = *((const u4*)shadow + i);
                }
            }
            if (OP == 0) {
#pragma unroll
                for (int k = 0; k < VEC_PER_LANE; ++k) {
                    const f4 wf = __builtin_bit_cast(f4, w[k]), ef = __builtin_bit_cast(f4, e[k]);
                    f4 r;
                    r.x = ema1(ef.x, wf.x, omd);
                    r.y = ema1(ef.y, wf.y, omd);
                    r.z = ema1(ef.z, wf.z, omd);
                    r.w = ema1(ef.w, wf.w, omd);
                    e[k] = __builtin_bit_cast(u4, r);
                }
            }
#pragma unroll
            for (int k = 0; k < VEC_PER_LANE; ++k) {
                const int i = tid + k * THREADS;
                if (i < nv) {
                    if (OP == 0) {
                        *((u4*)shadow + i) = e[k];
                    } else {
                        *((u4*)shadow + i) = w[k];
                        *((u4*)live + i) = e[k];
                    }
                }
            }
            FMRI_STORE_FENCE();
            const int i = (nv << 2) + tid;                            // the dword tail: at most three
            if (i < n) {
                const uint32_t wt = *((const uint32_t*)live + i), et = *((const uint32_t*)shadow + i);
                if (OP == 0) {
                    shadow[i] = ema1(__builtin_bit_cast(float, et), __builtin_bit_cast(float, wt), omd);
                } else {
                    *((uint32_t*)shadow + i) = wt;
                    *((uint32_t*)live + i) = et;
                }
            }
        } else {
            for (int i = tid; i < n; i += THREADS) {
                const uint32_t wt = *((const uint32_t*)live + i), et = *((const uint32_t*)shadow + i);
                if (OP == 0) {
                    shadow[i] = ema1(__builtin_bit_cast(float, et), __builtin_bit_cast(float, wt), omd);
                } else {
                    *((uint32_t*)shadow + i) = wt;
                    *((uint32_t*)live + i) = et;
                }
            }
        }
    }
}

}  // namespace

float ema_decay_at(int32_t t, int32_t start, float decay, int32_t warmup) { return decay_at(t, start, decay, warmup); }

int64_t ema_table_chunks(const void* segs_host, int nseg) {
    const fmri_ema_seg* segs = (const fmri_ema_seg*)segs_host;
    int64_t chunks = 0;
    for (int i = 0; i < nseg; ++i) {
        const fmri_ema_seg& s = segs[i];
        if (s.n < 0 || s.chunk0 != chunks) return E_BADARG;
        if (s.n > 0 && (!s.live || !s.shadow || (((uintptr_t)s.live | (uintptr_t)s.shadow) & 3))) return E_BADARG;
        chunks += (s.n + FMRI_EMA_CHUNK - 1) / FMRI_EMA_CHUNK;
    }
    return chunks;
}

int ema_launch(const void* segs_dev, int nseg, int64_t chunks, const void* state_dev, int op, hipStream_t st) {
    if (chunks < 1) return OK;                                        // nothing but empty segments
    const fmri_ema_seg* segs = (const fmri_ema_seg*)segs_dev;
    const fmri_ema_state* state = (const fmri_ema_state*)state_dev;
    const int64_t grid = chunks < 2048 ? chunks : 2048;
    if (op == 0)
        hipLaunchKernelGGL((ema_kernel<0>), dim3((unsigned)grid), dim3(THREADS), 0, st, segs, nseg, chunks, state);
    else
        hipLaunchKernelGGL((ema_kernel<1>), dim3((unsigned)grid), dim3(THREADS), 0, st, segs, nseg, chunks, state);
    return hipGetLastError() == hipSuccess ? OK : E_LAUNCH;
}

}  // namespace fmri
