// league.hip -- league bookkeeping on the device.
//
// mlg_league_record_runs: the episode results of one batched self-play run folded into the league's local payoff
// delta entry (home, away) in ONE launch, replacing a dozen elementwise / reduce launches of the host-side form.
// Restates _extract_result + _update_payoff (src/league/processes/training/league_experiment_process.py:85-105):
// per env, DRAW if the env says so or if both / no team won, else WIN / LOSS by the policy team's battle_won;
// GAMES += B unless the reference-compatible payoff is kept (the reference never increments GAMES, payoff.py).
#include <hip/hip_runtime.h>

#include "../../include/maleague.h"
#include "mlg_host.h"

namespace {

constexpr int kRecThreads = 1024;

// one block: lane-strided pass over the envs, wave ballots, a 16-wave LDS sum, thread 0 adds into the entry
__global__ void __launch_bounds__(kRecThreads) league_record_kernel(const int32_t* __restrict__ won,
                                                                    const int32_t* __restrict__ draw, int B,
                                                                    float* __restrict__ entry, int count_games) {
    __shared__ int part[kRecThreads / 64][3];
    int w = 0, l = 0, d = 0;
    // the run summary lives in pinned host memory (zero copy): a thread's loads are all issued before the first is
    // used -- one host round trip, where the strided loop waited for each element in turn
    constexpr int PER = 8;
    for (int b0 = threadIdx.x; b0 < B; b0 += PER * kRecThreads) {
        int wa[PER], wb[PER], dv[PER];
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int b = b0 + u * kRecThreads;
            wa[u] = b < B ? won[2 * b] : 0;
            wb[u] = b < B ? won[2 * b + 1] : 0;
            dv[u] = b < B ? draw[b] : 0;
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            if (b0 + u * kRecThreads >= B) break;
            const bool w0 = wa[u] != 0, w1 = wb[u] != 0;
            const bool dr = dv[u] != 0 || w0 == w1;
            w += !dr && w0;
            l += !dr && !w0;
            d += dr;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        w += __shfl_xor(w, m);
        l += __shfl_xor(l, m);
        d += __shfl_xor(d, m);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[wave][0] = w;
        part[wave][1] = l;
        part[wave][2] = d;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int sw = 0, sl = 0, sd = 0;
        for (int k = 0; k < kRecThreads / 64; ++k) {
            sw += part[k][0];
            sl += part[k][1];
            sd += part[k][2];
        }
        // PayoffEntry: GAMES 0, WIN 1, LOSS 2, DRAW 3 (the delta is private to this rank: plain read-modify-write)
        if (count_games) entry[0] += (float)B;
        entry[1] += (float)sw;
        entry[2] += (float)sl;
        entry[3] += (float)sd;
    }
}

// The mixture form: env b books into column group_col[b / 16]. One block of 16 waves; wave w owns the columns w,
// w + 16, ... and nobody else touches their entries. Per column the wave scans the group table 64 entries at a time
// and reads the 16 envs of up to four matching groups at once (one quarter-wave per group: the run summary may live
// in pinned host memory, so a wave's loads of one pass are issued together). Counts are integers; the 64 lane counts
// are added by a butterfly and lane 0 adds each total into the entry once.
__global__ void __launch_bounds__(kRecThreads) league_record_mix_kernel(const int32_t* __restrict__ won,
                                                                        const int32_t* __restrict__ draw, int B, int G,
                                                                        const int32_t* __restrict__ group_col,
                                                                        int n_cols, float* __restrict__ row,
                                                                        int64_t entry_stride, int count_games) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, le = lane & 15;
    for (int c = wave; c < n_cols; c += kRecThreads / 64) {
        int w = 0, l = 0, d = 0, n = 0;
        for (int g0 = 0; g0 < G; g0 += 64) {
            const int g = g0 + lane;
            unsigned long long m = __ballot(g < G && group_col[g] == c);
            while (m) {  // wave-uniform: up to four matching groups per pass, quarter q takes the q-th
                unsigned long long mq = m;
                for (int k = 0; k < q; ++k) mq &= mq - 1;
                const int b = mq ? (g0 + __ffsll((long long)mq) - 1) * 16 + le : B;
                if (b < B) {
                    const bool w0 = won[2 * b] != 0, w1 = won[2 * b + 1] != 0;
                    const bool dr = draw[b] != 0 || w0 == w1;
                    w += !dr && w0;
                    l += !dr && !w0;
                    d += dr;
                    n += 1;
                }
                for (int k = 0; k < 4 && m; ++k) m &= m - 1;
            }
        }
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            w += __shfl_xor(w, s);
            l += __shfl_xor(l, s);
            d += __shfl_xor(d, s);
            n += __shfl_xor(n, s);
        }
        if (lane == 0) {
            float* entry = row + (int64_t)c * entry_stride;
            if (count_games) entry[0] += (float)n;
            entry[1] += (float)w;
            entry[2] += (float)l;
            entry[3] += (float)d;
        }
    }
}

}  // namespace

extern "C" int mlg_league_record_runs_mix(const int32_t* won, const int32_t* draw, int32_t B, const int32_t* group_col,
                                          int32_t n_cols, float* row, int64_t entry_stride, int32_t count_games,
                                          void* stream) {
    MLG_REQUIRE(won && draw && group_col && row, "league_record_runs_mix: null pointer");
    MLG_REQUIRE(B >= 1 && n_cols >= 1, "league_record_runs_mix: B=%d n_cols=%d must be >= 1", B, n_cols);
    MLG_REQUIRE(entry_stride >= 4, "league_record_runs_mix: entry_stride=%lld < 4 (GAMES, WIN, LOSS, DRAW)",
                (long long)entry_stride);
    hipLaunchKernelGGL(league_record_mix_kernel, dim3(1), dim3(kRecThreads), 0, (hipStream_t)stream, won, draw, B,
                       (B + 15) / 16, group_col, n_cols, row, entry_stride, count_games);
    return mlg::check_launch("league_record_runs_mix");
}

extern "C" int mlg_league_record_runs(const int32_t* won, const int32_t* draw, int32_t B, float* entry,
                                      int32_t count_games, void* stream) {
    MLG_REQUIRE(won && draw && entry, "league_record_runs: null pointer");
    MLG_REQUIRE(B >= 1, "league_record_runs: B=%d", B);
    hipLaunchKernelGGL(league_record_kernel, dim3(1), dim3(kRecThreads), 0, (hipStream_t)stream, won, draw, B, entry,
                       count_games);
    return mlg::check_launch("league_record_runs");
}
