// Epoch-end schedules and the per-step training log of the fused steps (include/fmri_hip.h fmri_schedule for the
// semantics; fmri_hip/schedule.py).  Two scalar-sized kernels that bracket a step:
//
//   epoch_begin_kernel      one thread, the first launch of a fed step: reads the epoch of the batch about to be drawn from
//                           the feed's device state, moves the schedule there (FMRI_SCHEDULE_SEEK of the header -- the
//                           same inline code the host entry point runs) and stores the fp32 roundings where the optimizer
//                           and gate kernels read them.
//   trainlog_append_kernel  one wave, the last launch of a logged step: lane k copies source k into the ring row of this
//                           step, then lane 0 bumps the counter.
//
// Neither has anything to overlap or to tile: they exist so that an epoch boundary and a log line cost a launch inside
// the recorded graph instead of a host synchronisation between replays.
#include "../../include/fmri_hip.h"
#include "kernels.h"

namespace fmri {

namespace {

__global__ void epoch_begin_kernel(const int64_t* __restrict__ feed_state, fmri_schedule* sched, float* lr0, float* lr1,
                                   float* lr2, float* lr3, float* hp3, int64_t* epoch_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t e = feed_state[1];
    if (e < 0) e = 0;
    if (epoch_out) *epoch_out = e;
    if (!sched || sched->lr_step < 1) return;
    FMRI_SCHEDULE_SEEK(sched, e);
    float* const lr[FMRI_SCHED_MAX_LR] = {lr0, lr1, lr2, lr3};
#pragma unroll
    for (int i = 0; i < FMRI_SCHED_MAX_LR; ++i)
        if (lr[i]) *lr[i] = (float)sched->lr[i];
    if (hp3) {
        hp3[0] = (float)sched->lambda_mse;
        hp3[1] = (float)sched->equilibrium;
        hp3[2] = (float)sched->margin;
    }
}

__global__ __launch_bounds__(64) void trainlog_append_kernel(const void* const* __restrict__ src,
                                                             const int32_t* __restrict__ kind, int K,
                                                             float* __restrict__ ring, uint64_t capacity,
                                                             int64_t* counter) {
    const int k = threadIdx.x;
    const int64_t n = *counter;                          // every lane reads it in front of the barrier below
    if (k < K) {
        const void* p = src[k];
        const int t = kind[k];
        const float v = t == 0 ? *(const float*)p : t == 1 ? (float)*(const int32_t*)p : (float)*(const int64_t*)p;
        ring[((uint64_t)n % capacity) * (uint64_t)K + (uint64_t)k] = v;       // row < capacity, k < K: in bounds
    }
    __syncthreads();
    if (k == 0) *counter = n + 1;
}

}  // namespace

int epoch_begin_launch(const int64_t* feed_state, void* sched, float* lr0, float* lr1, float* lr2, float* lr3,
                       float* hp3, int64_t* epoch_out, hipStream_t st) {
    hipLaunchKernelGGL(epoch_begin_kernel, dim3(1), dim3(64), 0, st, feed_state, (fmri_schedule*)sched, lr0, lr1, lr2,
                       lr3, hp3, epoch_out);
    return hipGetLastError() == hipSuccess ? OK : E_LAUNCH;
}

int schedule_seek_host(void* sched, int64_t epoch, float* out7) {
    fmri_schedule* s = (fmri_schedule*)sched;
    FMRI_SCHEDULE_SEEK(s, epoch);
    if (out7) {
        for (int i = 0; i < FMRI_SCHED_MAX_LR; ++i) out7[i] = (float)s->lr[i];
        out7[4] = (float)s->lambda_mse;
        out7[5] = (float)s->equilibrium;
        out7[6] = (float)s->margin;
    }
    return OK;
}

int trainlog_append_launch(const void* const* src, const int32_t* kind, int K, float* ring, int64_t capacity,
                           int64_t* counter, hipStream_t st) {
    hipLaunchKernelGGL(trainlog_append_kernel, dim3(1), dim3(64), 0, st, src, kind, K, ring, (uint64_t)capacity, counter);
    return hipGetLastError() == hipSuccess ? OK : E_LAUNCH;
}

}  // namespace fmri
