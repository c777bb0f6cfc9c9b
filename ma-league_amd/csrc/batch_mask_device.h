// batch_mask_device.h -- the mask statistics of a sampled learner batch, computed by one workgroup of a learner's
// prologue launch (learner.hip prep_kernel block 0, refil_learner.hip prologue_kernel block 0). Restates the
// reference's mask and truncation (q_learner.py:58-60, 89-95; ma_experiment.py:235-239):
//   mask(b, t) = filled(b, t) * (1 - terminated(b, t - 1))   (t > 0; t = 0: filled(b, 0))
//   Te         = clamp(max_b sum_t filled(b, t), 2, T)           (max_t_filled)
//   msum[0]    = sum_{b, t < Te - 1} mask(b, t),  msum[1] = Te
//   mixlen[b]  = 1 + the last t < Te - 1 with mask(b, t) != 0    (0: none; REFIL only)
// A wave per episode (episodes wave, wave + waves, ... up to EPW per wave) with every load of all of the wave's
// episodes issued before the first is used -- one memory round trip, where the serial per-episode scans it replaces
// waited once per episode and 64-step chunk -- then ballots: each episode's filled count and live bits are written
// by one lane (no atomics on shared counters), Te is one atomicMax per episode. Every quantity is an integer count
// (exact in float). That path holds B <= waves * EPW episodes of T <= 32 * MLG_MS_TW steps (mask_stats_fits); any
// other shape takes batch_mask_scan, a wave per episode in turn over 64-step chunks, which produces the same
// counts and therefore the same floats bit for bit. Callers use batch_mask, which picks the path.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mlg {

constexpr int MLG_MS_BMAX = 256, MLG_MS_TW = 4;

struct MaskStatsLds {
    int cnt[MLG_MS_BMAX];                   // filled steps per episode
    uint32_t live[MLG_MS_BMAX][MLG_MS_TW];  // mask(b, t) != 0 as bits
    int te, total;
};

template <int EPW>
__host__ __device__ constexpr bool mask_stats_fits(int B, int T, int waves) {
    return B <= MLG_MS_BMAX && B <= waves * EPW && T <= 32 * MLG_MS_TW;
}

// slot(b): the episode's row in the batch storage (sampled views)
template <int EPW, class SlotFn>
__device__ void batch_mask_stats(const int64_t* __restrict__ filled, const uint8_t* __restrict__ term, int T1,
                                 SlotFn slot, int B, int T, float* __restrict__ msum, float* __restrict__ mixlen,
                                 MaskStatsLds& S) {
    static_assert(MLG_MS_TW == 4, "two 64-step chunks per episode");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    if (tid == 0) S.te = S.total = 0;
    int64_t f[EPW][2];
    uint8_t tp[EPW][2];
#pragma unroll
    for (int k = 0; k < EPW; ++k) {  // every load of the wave's episodes before the first use
        const int b = wave + nw * k;
        const bool eb = b < B;
        const int64_t base = slot(eb ? b : 0) * T1;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int t = 64 * c + lane;
            const bool in = eb && t < T;
            f[k][c] = in ? filled[base + t] : 0;
            tp[k][c] = (in && t > 0) ? term[base + t - 1] : (uint8_t)0;
        }
    }
    __syncthreads();  // te / total initialised
#pragma unroll
    for (int k = 0; k < EPW; ++k) {
        const int b = wave + nw * k;
        if (b >= B) break;  // wave-uniform
        const uint64_t f0 = __ballot(f[k][0] != 0), f1 = __ballot(f[k][1] != 0);
        const uint64_t l0 = __ballot(f[k][0] != 0 && tp[k][0] == 0), l1 = __ballot(f[k][1] != 0 && tp[k][1] == 0);
        if (lane == 0) {
            const int n = __popcll(f0) + __popcll(f1);
            S.cnt[b] = n;
            S.live[b][0] = (uint32_t)l0;
            S.live[b][1] = (uint32_t)(l0 >> 32);
            S.live[b][2] = (uint32_t)l1;
            S.live[b][3] = (uint32_t)(l1 >> 32);
            atomicMax(&S.te, n);
        }
    }
    __syncthreads();
    const int Te = min(max(S.te, 2), T);
    for (int b = tid; b < B; b += blockDim.x) {
        int c = 0, last = -1;
#pragma unroll
        for (int w = 0; w < MLG_MS_TW; ++w) {
            const int lim = Te - 1 - 32 * w;  // steps t < Te - 1 of this word
            const uint32_t keep = lim >= 32 ? 0xFFFFFFFFu : (lim <= 0 ? 0u : ((1u << lim) - 1u));
            const uint32_t m = S.live[b][w] & keep;
            c += __builtin_popcount(m);
            if (m) last = 32 * w + 31 - __builtin_clz(m);
        }
        if (c) atomicAdd(&S.total, c);
        if (mixlen) mixlen[b] = (float)(last + 1);
    }
    __syncthreads();
    if (tid == 0) {
        msum[0] = (float)S.total;
        msum[1] = (float)Te;
    }
}

// Any B and T: the same statistics with a wave per episode in turn (episodes wave, wave + waves, ...) and one memory
// round trip per 64-step chunk. Uses S.te / S.total only.
template <class SlotFn>
__device__ void batch_mask_scan(const int64_t* __restrict__ filled, const uint8_t* __restrict__ term, int T1,
                                SlotFn slot, int B, int T, float* __restrict__ msum, float* __restrict__ mixlen,
                                MaskStatsLds& S) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    if (tid == 0) S.te = S.total = 0;
    __syncthreads();
    for (int b = wave; b < B; b += nw) {  // filled steps counted with ballots
        const int64_t base = slot(b) * T1;
        int n = 0;
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int t = t0 + lane;
            n += __popcll(__ballot(t < T && filled[base + t] != 0));
        }
        if (lane == 0) atomicMax(&S.te, n);
    }
    __syncthreads();
    const int Te = min(max(S.te, 2), T);
    for (int b = wave; b < B; b += nw) {
        const int64_t base = slot(b) * T1;
        int c = 0, last = -1;
        for (int t0 = 0; t0 < Te - 1; t0 += 64) {
            const int t = t0 + lane;
            const bool live = t < Te - 1 && filled[base + t] != 0 && (t == 0 || term[base + t - 1] == 0);
            const uint64_t m = __ballot(live);
            c += __popcll(m);
            if (m) last = t0 + 63 - __builtin_clzll(m);
        }
        if (lane == 0) {
            if (c) atomicAdd(&S.total, c);
            if (mixlen) mixlen[b] = (float)(last + 1);
        }
    }
    __syncthreads();
    if (tid == 0) {
        msum[0] = (float)S.total;
        msum[1] = (float)Te;
    }
}

// The statistics by whichever path holds the batch (workgroup-uniform choice). mixlen may be null.
template <int EPW, class SlotFn>
__device__ __forceinline__ void batch_mask(const int64_t* __restrict__ filled, const uint8_t* __restrict__ term, int T1,
                                           SlotFn slot, int B, int T, float* __restrict__ msum,
                                           float* __restrict__ mixlen, MaskStatsLds& S) {
    if (mask_stats_fits<EPW>(B, T, blockDim.x >> 6))
        batch_mask_stats<EPW>(filled, term, T1, slot, B, T, msum, mixlen, S);
    else
        batch_mask_scan(filled, term, T1, slot, B, T, msum, mixlen, S);
}

// max_t_filled of the batch (msum[1]): the learners use transitions t < t_eff - 1 only; the sequential kernels stop
// there and the per-t kernels skip the steps beyond
__device__ __forceinline__ int t_eff(const float* msum) { return (int)msum[1]; }

}  // namespace mlg
