// Device-side training-state ring (include/fmri_hip.h fmri_state_copy for the semantics; fmri_hip/state.py).
//
//   state_copy_kernel   one many-segment copy, live tensors <-> one slot of the ring.  A chunk (FMRI_STATE_CHUNK bytes of
//                       one segment) is one block's unit of work; blocks walk the chunks grid-stride and find a chunk's
//                       segment by binary search over the table's running chunk counts.  With a feed state and `every`
//                       the launch is predicated: every block reads the same [epoch, cursor] words, which nothing in the
//                       launch writes, and returns at once when the epoch that just ended is not one to keep.
//
// Nothing to tile and nothing to reuse: the kernel is a device-to-device copy whose only job is to keep 4 x 16 bytes per
// lane in flight and to touch no byte outside a segment.  The slot side of the copy is non-temporal -- nobody on the device
// reads a slot again -- unless fmri_state_nontemporal(0) says otherwise (profiles/state_ring.md has the measurement).
#include <atomic>

#include "../../include/fmri_hip.h"
#include "common.h"
#include "kernels.h"

namespace fmri {

namespace {

typedef uint32_t u4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;
constexpr int VEC_PER_LANE = FMRI_STATE_CHUNK / (THREADS * 16);      // 16-byte accesses per lane and chunk
static_assert(VEC_PER_LANE * THREADS * 16 == FMRI_STATE_CHUNK, "a chunk is a whole number of 16-byte accesses per lane");

template <bool NT, typename T>
__device__ __forceinline__ T slot_load(const T* p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    return *p;
}
template <bool NT, typename T>
__device__ __forceinline__ void slot_store(T* p, T v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// DIR 0: live -> slot, DIR 1: slot -> live; NT: the slot side's accesses are non-temporal
template <int DIR, bool NT>
__global__ __launch_bounds__(THREADS) void state_copy_kernel(const fmri_state_seg* __restrict__ segs, int nseg,
                                                             int64_t chunks, uint8_t* ring, int64_t slot_bytes,
                                                             const int64_t* __restrict__ feed_state, int every,
                                                             int capacity, uint64_t fingerprint,
                                                             const int64_t* __restrict__ log_counter) {
    int64_t slot = capacity, epoch = -1, cursor = -1;
    if (feed_state) {
        epoch = feed_state[1];
        cursor = feed_state[2];
        if (every > 0) {
            if (cursor != 0 || epoch < 1 || (epoch - 1) % every != 0) return;
            slot = ((epoch - 1) / every) % capacity;
        }
    }
    uint8_t* const base = ring + slot * slot_bytes;                   // slot <= capacity: inside the ring (host check)
    const int tid = threadIdx.x;
    if (DIR == 0 && blockIdx.x == 0 && tid == 0) {
        int64_t* h = (int64_t*)base;
        h[0] = FMRI_STATE_MAGIC;
        h[1] = (int64_t)fingerprint;
        h[2] = epoch;
        h[3] = cursor;
        h[4] = log_counter ? *log_counter : -1;
        h[5] = slot_bytes - FMRI_STATE_HEADER;
        h[6] = 0;
        h[7] = 0;
    }
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        // the last segment whose first chunk is <= c (empty segments share their successor's chunk0 and sort in front)
        int lo = 0, hi = nseg - 1;
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (segs[mid].chunk0 <= c) lo = mid;
            else hi = mid - 1;
        }
        const fmri_state_seg s = segs[lo];
        const int64_t b0 = (c - s.chunk0) * FMRI_STATE_CHUNK;         // < s.bytes: c is one of the segment's chunks
        const int n = (int)(s.bytes - b0 < FMRI_STATE_CHUNK ? s.bytes - b0 : FMRI_STATE_CHUNK);
        uint8_t* const live = (uint8_t*)s.live + b0;
        uint8_t* const held = base + s.offset + b0;
        if (((uintptr_t)s.live & 15) == 0) {
            // both sides 16-byte aligned (offsets and chunks are multiples of 16): 16 bytes per lane, every load of the
            // chunk issued in front of the first store
            const int nv = n >> 4;
            u4 v[VEC_PER_LANE];
#pragma unroll
            for (int k = 0; k < VEC_PER_LANE; ++k) {
                const int i = tid + k * THREADS;
                if (i < nv) v[k] = DIR == 0 ? *((const u4*)live + i) : slot_load<NT>((const u4*)held + i);
            }
#pragma unroll
            for (int k = 0; k < VEC_PER_LANE; ++k) {
                const int i = tid + k * THREADS;
                if (i < nv) {
                    if (DIR == 0) slot_store<NT>((u4*)held + i, v[k]);
                    else *((u4*)live + i) = v[k];
                }
            }
            FMRI_STORE_FENCE();
            const int i = (nv << 2) + tid;                            // the dword tail: at most three
            if (i < (n >> 2)) {
                if (DIR == 0) slot_store<NT>((uint32_t*)held + i, *((const uint32_t*)live + i));
                else *((uint32_t*)live + i) = slot_load<NT>((const uint32_t*)held + i);
            }
        } else {
            for (int i = tid; i < (n >> 2); i += THREADS) {
                if (DIR == 0) slot_store<NT>((uint32_t*)held + i, *((const uint32_t*)live + i));
                else *((uint32_t*)live + i) = slot_load<NT>((const uint32_t*)held + i);
            }
        }
    }
}

// the slot side's access policy: 1 non-temporal (the default: 0.085-0.088 ms against 0.108-0.111 ms per launch at
// Stage-I's 270 MB, profiles/state_ring.md), 0 plain
std::atomic<int> g_nontemporal{1};

}  // namespace

int state_nontemporal(int on) {
    return on < 0 ? g_nontemporal.load() : g_nontemporal.exchange(on ? 1 : 0);
}

int64_t state_layout(const int64_t* bytes, int nseg, int64_t* offsets_out) {
    int64_t at = FMRI_STATE_HEADER;
    for (int i = 0; i < nseg; ++i) {
        if (bytes[i] < 0 || (bytes[i] & 3)) return E_BADARG;
        if (offsets_out) offsets_out[i] = at;
        at += (bytes[i] + 15) & ~(int64_t)15;
    }
    return at;
}

int64_t state_table_chunks(const void* segs_host, int nseg, int64_t slot_bytes) {
    const fmri_state_seg* segs = (const fmri_state_seg*)segs_host;
    int64_t at = FMRI_STATE_HEADER, chunks = 0;
    for (int i = 0; i < nseg; ++i) {
        const fmri_state_seg& s = segs[i];
        if (s.bytes < 0 || (s.bytes & 3) || (s.offset & 15) || s.offset < at || s.chunk0 != chunks) return E_BADARG;
        if (s.bytes > 0 && (!s.live || ((uintptr_t)s.live & 3))) return E_BADARG;
        if (s.bytes > slot_bytes - s.offset) return E_BADARG;
        at = s.offset + s.bytes;
        chunks += (s.bytes + FMRI_STATE_CHUNK - 1) / FMRI_STATE_CHUNK;
    }
    return chunks;
}

int state_copy_launch(const void* segs_dev, int nseg, int64_t chunks, void* ring, int64_t slot_bytes, int dir,
                      const int64_t* feed_state, int every, int capacity, uint64_t fingerprint,
                      const int64_t* log_counter, hipStream_t st) {
    const fmri_state_seg* segs = (const fmri_state_seg*)segs_dev;
    const int64_t grid = chunks < 1 ? 1 : chunks < 2048 ? chunks : 2048;      // one block writes the header of an empty table
    const bool nt = g_nontemporal.load() != 0;
#define FMRI_STATE_LAUNCH(DIR, NT)                                                                                   \
    hipLaunchKernelGGL((state_copy_kernel<DIR, NT>), dim3((unsigned)grid), dim3(THREADS), 0, st, segs, nseg, chunks, \
                       (uint8_t*)ring, slot_bytes, feed_state, every, capacity, fingerprint, log_counter)
    if (dir == 0) {
        if (nt) FMRI_STATE_LAUNCH(0, true);
        else FMRI_STATE_LAUNCH(0, false);
    } else {
        if (nt) FMRI_STATE_LAUNCH(1, true);
        else FMRI_STATE_LAUNCH(1, false);
    }
#undef FMRI_STATE_LAUNCH
    return hipGetLastError() == hipSuccess ? OK : E_LAUNCH;
}

}  // namespace fmri
