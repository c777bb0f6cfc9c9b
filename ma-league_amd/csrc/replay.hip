// replay.hip -- prioritized episode replay on the device: the stratified draw over the replay ring's
// priority vector, the priorities of newly written slots, and the priorities of the slots a train call sampled.
// Restates the reference's Memory / BinarySumTree (src/marl/components/replay_buffers/prioritized_replay_buffer.py:
// 8-135: priority (|err| + e)^a, stratified draws, weights (n p / total)^-beta / max) on a flat priority vector in slot
// order; the three defects that keep the reference's PrioritizedReplayBuffer from running are listed in DESIGN.md §7.
//   mlg_per_sample  one workgroup: fp64 inclusive scan of the live priorities (wave64 shuffles in the wave, LDS across
//                   the waves, a carry across 1024-slot chunks), B binary searches, the normalised weights
//   mlg_per_insert  priorities of `count` ring slots from slot0: the device maximum, or (|err| + e)^a
//   mlg_per_update  priorities of the sampled slots from the learner's per-episode errors; raises the maximum
// Every sum and maximum is taken in a fixed order, no float atomics: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include "../../include/maleague.h"
#include "mlg_device.h"
#include "mlg_host.h"

namespace {

enum { MLG_PURPOSE_PER = 6 };

constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr int kLdsSlots = 6144;   // the scan stays in LDS up to this many live slots (48 KB of doubles)
constexpr int kMaxSlots = 1 << 20;
constexpr int kMaxBatch = 4096;   // draws per call: 4 per thread, and the 12-bit index field of mlg_ctr
constexpr int kDraws = kMaxBatch / kThreads;

__device__ __forceinline__ double wave_scan_incl(double v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const double o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ double block_max(double v, double* red, int tid) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
    __syncthreads();  // red may still be read from an earlier use
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double r = red[0];
    for (int k = 1; k < (int)(blockDim.x >> 6); ++k) r = fmax(r, red[k]);
    return r;
}

// cum[j] = prio[0] + .. + prio[j] in fp64: chunk of 1024 slots at a time, thread i one slot; the wave's inclusive scan,
// the sums of the waves before it in ascending order, then the carry of the chunks before.
__global__ void __launch_bounds__(kThreads) per_sample_kernel(const float* __restrict__ prio, int n, int B, uint64_t seed,
                                                              uint32_t draw, double beta, int32_t* __restrict__ rows,
                                                              float* __restrict__ is_weight, double* __restrict__ scan_ws) {
    __shared__ double lcum[kLdsSlots];
    __shared__ double wsum[kWaves];
    __shared__ double red[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double* cum = n <= kLdsSlots ? lcum : scan_ws;
    double carry = 0.0;
    for (int j0 = 0; j0 < n; j0 += kThreads) {
        const int j = j0 + tid;
        const double v = wave_scan_incl(j < n ? (double)prio[j] : 0.0, lane);
        if (lane == 63) wsum[wv] = v;
        __syncthreads();
        double before = carry;
        for (int k = 0; k < wv; ++k) before += wsum[k];
        if (j < n) cum[j] = before + v;
        for (int k = 0; k < kWaves; ++k) carry += wsum[k];  // every thread alike: the chunk's total onto the carry
        __syncthreads();  // wsum is rewritten by the next chunk
    }
    if (cum == scan_ws) __threadfence_block();
    __syncthreads();
    const double total = cum[n - 1];
    int jr[kDraws];
    double wr[kDraws];
    double wmax = 0.0;
#pragma unroll
    for (int q = 0; q < kDraws; ++q) {
        const int i = tid + q * kThreads;
        jr[q] = 0;
        wr[q] = 0.0;
        if (i >= B) continue;
        const double u = (double)mlg_u01(mlg_rng(seed, mlg_ctr(draw, 0u, MLG_PURPOSE_PER, (uint32_t)i)));
        const double s = ((double)i + u) * total / (double)B;
        int lo = 0, hi = n - 1;  // the first slot whose inclusive cumulative priority is >= s (the last if none is)
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cum[mid] >= s) hi = mid;
            else lo = mid + 1;
        }
        jr[q] = lo;
        wr[q] = pow((double)n * (double)prio[lo] / total, -beta);
        wmax = fmax(wmax, wr[q]);
    }
    wmax = block_max(wmax, red, tid);
#pragma unroll
    for (int q = 0; q < kDraws; ++q) {
        const int i = tid + q * kThreads;
        if (i >= B) continue;
        rows[i] = jr[q];
        is_weight[i] = (float)(wr[q] / wmax);
    }
}

__device__ __forceinline__ float priority_of(float err, double e, double a) {
    return (float)pow((double)fabsf(err) + e, a);
}

// one workgroup; the maximum is read before and stored after every slot write by thread 0
__global__ void __launch_bounds__(256) per_insert_kernel(float* __restrict__ prio, int ring, int slot0, int count,
                                                         const float* __restrict__ errors, double e, double a,
                                                         float* __restrict__ max_prio) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const float pmax = *max_prio;
    double mx = 0.0;
    for (int k = tid; k < count; k += blockDim.x) {
        const float p = errors ? priority_of(errors[k], e, a) : pmax;
        prio[(slot0 + k) % ring] = p;
        mx = fmax(mx, (double)p);
    }
    mx = block_max(mx, red, tid);
    if (tid == 0 && (float)mx > pmax) *max_prio = (float)mx;
}

__global__ void __launch_bounds__(256) per_update_kernel(float* __restrict__ prio, int n_slots,
                                                         const int32_t* __restrict__ rows,
                                                         const float* __restrict__ td_abs, int B, double e, double a,
                                                         float* __restrict__ max_prio) {
    __shared__ double red[4];
    const int tid = threadIdx.x;
    const float pmax = *max_prio;
    double mx = 0.0;
    for (int b = tid; b < B; b += blockDim.x) {
        const int slot = rows ? rows[b] : b;
        if (slot < 0 || slot >= n_slots) continue;  // a slot map this call cannot check on the host
        const float p = priority_of(td_abs[b], e, a);  // duplicated slots: the same episode, the same error, one value
        prio[slot] = p;
        mx = fmax(mx, (double)p);
    }
    mx = block_max(mx, red, tid);
    if (tid == 0 && (float)mx > pmax) *max_prio = (float)mx;
}

}  // namespace

extern "C" int32_t mlg_per_lds_slots(void) { return kLdsSlots; }
extern "C" int32_t mlg_per_max_slots(void) { return kMaxSlots; }

extern "C" int mlg_per_sample(const float* priorities, int32_t n_live, int32_t B, uint64_t seed, uint32_t draw,
                              double beta, int32_t* rows, float* is_weight, double* scan_workspace,
                              int64_t scan_workspace_doubles, void* stream) {
    MLG_REQUIRE(priorities && rows && is_weight, "per_sample: null pointer");
    MLG_REQUIRE(n_live >= 1 && n_live <= kMaxSlots, "per_sample: episodes_in_buffer=%d unsupported (1..%d)", n_live,
                kMaxSlots);
    MLG_REQUIRE(B >= 1 && B <= kMaxBatch, "per_sample: batch_size=%d unsupported (1..%d)", B, kMaxBatch);
    MLG_REQUIRE(beta >= 0.0 && beta <= 1.0, "per_sample: beta=%g outside [0, 1]", beta);
    if (n_live > kLdsSlots)
        MLG_REQUIRE(scan_workspace && scan_workspace_doubles >= n_live && mlg::aligned16(scan_workspace),
                    "per_sample: episodes_in_buffer=%d > %d needs scan_workspace of that many doubles (got %lld)", n_live,
                    kLdsSlots, (long long)(scan_workspace ? scan_workspace_doubles : 0));
    hipLaunchKernelGGL(per_sample_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, priorities, n_live, B, seed,
                       draw, beta, rows, is_weight, scan_workspace);
    return mlg::check_launch("per_sample");
}

extern "C" int mlg_per_insert(float* priorities, int32_t ring_size, int32_t slot0, int32_t count, const float* errors,
                              double e, double a, float* max_priority, void* stream) {
    MLG_REQUIRE(priorities && max_priority, "per_insert: null pointer");
    MLG_REQUIRE(ring_size >= 1 && slot0 >= 0 && slot0 < ring_size, "per_insert: slot0=%d outside the ring of %d slots",
                slot0, ring_size);
    MLG_REQUIRE(count >= 1 && count <= ring_size, "per_insert: count=%d unsupported (1..ring_size=%d)", count, ring_size);
    MLG_REQUIRE(e >= 0.0 && a >= 0.0, "per_insert: e=%g a=%g must not be negative", e, a);
    hipLaunchKernelGGL(per_insert_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, priorities, ring_size, slot0, count,
                       errors, e, a, max_priority);
    return mlg::check_launch("per_insert");
}

extern "C" int mlg_per_update(float* priorities, int32_t n_slots, const int32_t* rows, const float* td_abs, int32_t B,
                              double e, double a, float* max_priority, void* stream) {
    MLG_REQUIRE(priorities && td_abs && max_priority, "per_update: null pointer");
    MLG_REQUIRE(n_slots >= 1 && B >= 1, "per_update: n_slots=%d B=%d", n_slots, B);
    MLG_REQUIRE(rows || B <= n_slots, "per_update: identity rows need B=%d <= n_slots=%d", B, n_slots);
    MLG_REQUIRE(e >= 0.0 && a >= 0.0, "per_update: e=%g a=%g must not be negative", e, a);
    hipLaunchKernelGGL(per_update_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, priorities, n_slots, rows, td_abs,
                       B, e, a, max_priority);
    return mlg::check_launch("per_update");
}
