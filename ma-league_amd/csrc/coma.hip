// coma.hip -- COMA (algs/coma.yaml): the policy output of the MAC (softmax + epsilon floor), multinomial action
// selection on the counter RNG, the critic training pipeline (target pass, TD(lambda), one optimizer step per
// timestep) and the actor loss with its gradient.
#include "coma_device.h"
#include "mlg_host.h"

namespace {

constexpr int CH = 128;    // critic hidden width (critics/coma.py:18-20 hard-codes it)
constexpr int CLD = 132;   // LDS row stride of a 16 x 128 activation tile
constexpr int CMAXA = 96;  // largest n_actions the critic kernels hold in six 16-wide tiles

// ---- MultiAgentController._softmax ----------------------------------------------------------------------------
// One thread per row; every sum runs over k in ascending order.
template <bool BACKWARD>
__global__ void policy_probs_kernel(const float* __restrict__ logits, const int32_t* __restrict__ avail,
                                    const float* __restrict__ g, int R, int A, float eps, int mask, int test_mode,
                                    float* __restrict__ out) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const float* x = logits + (int64_t)r * A;
    const int32_t* av = avail + (int64_t)r * A;
    float* o = out + (int64_t)r * A;
    float mx = -INFINITY;
    int K = 0;
    for (int k = 0; k < A; ++k) {
        const bool off = mask && av[k] == 0;
        K += !off;
        mx = fmaxf(mx, off ? -1e10f : x[k]);
    }
    if (mask && K == 0 && !test_mode) {  // every entry is zeroed by the final masked assignment (eps / 0 never shows)
        for (int k = 0; k < A; ++k) o[k] = 0.f;
        return;
    }
    float s = 0.f;
    for (int k = 0; k < A; ++k) s += expf(((mask && av[k] == 0) ? -1e10f : x[k]) - mx);
    const float keep = test_mode ? 1.f : 1.f - eps;
    if (!BACKWARD) {
        const float floor_p = test_mode ? 0.f : eps / (float)(mask ? K : A);
        for (int k = 0; k < A; ++k) {
            const bool off = mask && av[k] == 0;
            const float p = expf((off ? -1e10f : x[k]) - mx) / s;
            // the reference zeroes unavailable entries in train mode only; in test mode they are exp(-1e10 - mx) / s:
            // 0 next to an available action, 1 / A in a row without one
            o[k] = test_mode ? p : (off ? 0.f : keep * p + floor_p);
        }
        return;
    }
    // d logits_k = y_k (dy_k - sum_j dy_j y_j), dy = keep * g with the zeroed outputs passing nothing; a logit
    // overwritten by the -1e10 assignment gets no gradient
    const float* gr = g + (int64_t)r * A;
    float dot = 0.f;
    for (int k = 0; k < A; ++k) {
        const bool off = mask && av[k] == 0;
        const float y = expf((off ? -1e10f : x[k]) - mx) / s;
        dot += off ? 0.f : keep * gr[k] * y;
    }
    for (int k = 0; k < A; ++k) {
        const bool off = mask && av[k] == 0;
        const float y = expf((off ? -1e10f : x[k]) - mx) / s;
        o[k] = off ? 0.f : y * (keep * gr[k] - dot);
    }
}

// ---- MultinomialActionSelector.select ---------------------------------------------------------------------------
__global__ void select_multinomial_kernel(const float* __restrict__ probs, const int32_t* __restrict__ avail, int R,
                                          int A, int n_agents, const uint64_t* __restrict__ keys,
                                          const uint32_t* __restrict__ episodes, int t, int greedy,
                                          int64_t* __restrict__ actions) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const float* p = probs + (int64_t)r * A;
    const int32_t* av = avail + (int64_t)r * A;
    int act = 0;
    if (greedy) {
        float bv = -INFINITY;
        bool found = false;
        for (int k = 0; k < A; ++k)
            if (av[k] != 0 && (!found || p[k] > bv)) { bv = p[k]; act = k; found = true; }
    } else {
        float total = 0.f;
        for (int k = 0; k < A; ++k) total += av[k] != 0 ? p[k] : 0.f;
        const int env = r / n_agents, n = r % n_agents;
        const uint32_t ep = episodes ? episodes[env] : 0u;
        const float u = mlg_u01(mlg_rng(keys[env], mlg_ctr(ep, (uint32_t)t, MLG_PURPOSE_POLICY, (uint32_t)n)));
        const float thr = u * total;
        float run = 0.f;
        int last = 0;
        bool hit = false;
        for (int k = 0; k < A; ++k) {
            if (av[k] == 0) continue;
            last = k;
            run += p[k];
            if (!hit && run > thr) { act = k; hit = true; }
        }
        if (!hit) act = last;
    }
    actions[r] = act;
}

// Sum of v over the workgroup's threads in a fixed order (a binary tree over the thread index); every thread gets it.
// blockDim.x is a power of two <= 256; `red` holds 256 floats.
__device__ float block_sum(float v, float* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// block_sum in double: the actor loss's three sums run over every (b, t, n) row of the batch, so they are carried in
// double and rounded to fp32 once (the rows' own terms are fp32).
__device__ double block_sum_f64(double v, double* red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// ---- the actor loss (coma_learner.py:75-96) and d loss / d pi ---------------------------------------------------
__global__ void __launch_bounds__(256) coma_policy_loss_kernel(const float* __restrict__ pi,
                                                               const int32_t* __restrict__ avail,
                                                               const int64_t* __restrict__ actions,
                                                               const float* __restrict__ q_vals,
                                                               const float* __restrict__ mask, int rows, int N, int A,
                                                               float* __restrict__ out, float* __restrict__ d_pi) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double m = 0.0;
    for (int i = tid; i < rows; i += 256) m += (double)mask[i];
    const double msum64 = (double)N * block_sum_f64(m, red);
    const float msum = (float)msum64;
    double s_loss = 0.0, s_adv = 0.0, s_max = 0.0;
    const int R = rows * N;
    for (int r = tid; r < R; r += 256) {
        const float* p = pi + (int64_t)r * A;
        const int32_t* av = avail + (int64_t)r * A;
        const float* q = q_vals + (int64_t)r * A;
        float* d = d_pi + (int64_t)r * A;
        const float mk = mask[r / N];
        const int a = (int)actions[r];
        float s = 0.f;
        for (int k = 0; k < A; ++k) s += av[k] != 0 ? p[k] : 0.f;
        float base = 0.f, pmax = 0.f;
        for (int k = 0; k < A; ++k) {
            const float pn = (av[k] != 0 && s != 0.f) ? p[k] / s : 0.f;
            base += pn * q[k];
            pmax = fmaxf(pmax, pn);
        }
        const bool a_ok = a >= 0 && a < A && av[a] != 0 && s != 0.f;
        const float pt_raw = a_ok ? p[a] / s : 0.f;
        const float pt = mk == 0.f ? 1.f : pt_raw;
        const float adv = ((a >= 0 && a < A) ? q[a] : 0.f) - base;
        s_loss += (double)(logf(pt) * adv * mk);
        s_adv += (double)(adv * mk);
        s_max += (double)(pmax * mk);
        // d/d pi_k of -(mk adv / msum) log(pi_a / s) over the available k: -(mk adv / msum) (delta_ak / pi_a - 1 / s)
        const float gk = (mk != 0.f && a_ok && pt_raw > 0.f) ? -(mk * adv) / msum : 0.f;
        for (int k = 0; k < A; ++k) {
            float v = 0.f;
            if (gk != 0.f && av[k] != 0) v = gk * ((k == a ? 1.f / p[a] : 0.f) - 1.f / s);
            d[k] = v;
        }
    }
    const double t_loss = block_sum_f64(s_loss, red);
    const double t_adv = block_sum_f64(s_adv, red);
    const double t_max = block_sum_f64(s_max, red);
    if (tid == 0) {
        out[0] = (float)(-t_loss / msum64);
        out[1] = (float)(t_adv / msum64);
        out[2] = (float)(t_max / msum64);
        out[3] = msum;
    }
}

// ---- the critic pipeline ----------------------------------------------------------------------------------------
struct ComaDev {
    MlgBatch bt;
    int B, T, N, A, DO, S, D;
    // workspace
    float* tq;        // [B][T][N] the target critic's taken Q
    float* masks;     // [B][T-1]
    float* masksum;   // [T-1] sum_b mask[b, t]
    float* h1;        // [R][128] relu(fc1)
    float* h2;        // [R][128] relu(fc2)
    float* d1;        // [R][128] d loss / d fc1 pre-activation
    float* d2;        // [R][128] d loss / d fc2 pre-activation
    float* d3;        // [R] d loss / d q_taken
    float* rowstats;  // [R][4] (mask td)^2, |mask td|, q_taken mask, target mask
    float* partial;   // [grad blocks] sums of squared gradients
    float* q_vals;
    float* targets;
    float* stats;
    int64_t* counters;
};

struct ComaOffsets {
    int64_t w1, b1, w2, b2, w3, b3, total;
};
__host__ __device__ inline ComaOffsets coma_offsets(int D, int A) {
    ComaOffsets o;
    o.w1 = 0;
    o.b1 = o.w1 + (int64_t)CH * D;
    o.w2 = o.b1 + CH;
    o.b2 = o.w2 + CH * CH;
    o.w3 = o.b2 + CH;
    o.b3 = o.w3 + (int64_t)A * CH;
    o.total = o.b3 + A;
    return o;
}

__device__ __forceinline__ int coma_slot(const MlgBatch& bt, int b) { return bt.rows ? bt.rows[b] : b; }

// Element k of the critic input of row (slot, t, n) (critics/coma.py:29-61).
__device__ __forceinline__ float critic_x(const ComaDev& c, int slot, int t, int n, int k) {
    const int64_t st = (int64_t)slot * c.bt.T1 + t;
    if (k < c.S) return c.bt.state[st * c.S + k];
    k -= c.S;
    if (k < c.DO) return c.bt.obs[(st * c.N + n) * c.DO + k];
    k -= c.DO;
    const int NA = c.N * c.A;
    if (k < NA) return (k / c.A == n) ? 0.f : c.bt.actions_onehot[st * NA + k];
    k -= NA;
    if (k < NA) return t > 0 ? c.bt.actions_onehot[(st - 1) * NA + k] : 0.f;
    k -= NA;
    return k == n ? 1.f : 0.f;
}

// acc[ot] (16 output features x 16 rows, mlg_device.h orientation: lane l, reg r = feature 16 ot + 4 (l >> 4) + r of
// row l & 15) = bias + W x over K inputs; W element (o, k) at W[o * so + k * sk], x of row `col` from xs(k).
constexpr int DENSE_KB = 32;  // inputs per partial chain of dense16 (a multiple of 4)
template <int OT, class XF>
__device__ __forceinline__ void dense16(floatx4 (&acc)[OT], const float* __restrict__ W, int64_t so, int64_t sk,
                                        const float* __restrict__ bias, int O, int K, int lane, XF xs) {
    const int col = lane & 15, g = lane >> 4;
#pragma unroll
    for (int ot = 0; ot < OT; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = 16 * ot + 4 * g + r;
            acc[ot][r] = (bias && o < O) ? bias[o] : 0.f;
        }
    // Blocked sum: DENSE_KB inputs at a time go into a fresh chain that is then added to the total, so the rounding
    // error grows with the number of blocks and the block length, not with K (fc1 has K up to S + d_obs + 2 N A + N in
    // the thousands). One sequential chain over K = 400 was 4-5x further from float64 than a blocked fp32 sum.
    for (int kb = 0; kb < K; kb += DENSE_KB) {
        floatx4 part[OT];
#pragma unroll
        for (int ot = 0; ot < OT; ++ot) part[ot] = floatx4{0.f, 0.f, 0.f, 0.f};
        const int ke = kb + DENSE_KB < K ? kb + DENSE_KB : K;
        for (int k0 = kb; k0 < ke; k0 += 4) {
            const int k = k0 + g;
            const bool kin = k < K;
            const float x = kin ? xs(k) : 0.f;
#pragma unroll
            for (int ot = 0; ot < OT; ++ot) {
                const int o = 16 * ot + col;
                const float w = (kin && o < O) ? W[o * so + k * sk] : 0.f;
                part[ot] = mfma4(w, x, part[ot]);
            }
        }
#pragma unroll
        for (int ot = 0; ot < OT; ++ot) acc[ot] += part[ot];
    }
}

struct CriticLds {
    float h1[16 * CLD];
    float h2[16 * CLD];
    float d2[16 * CLD];
    float q[16 * (CMAXA + 1)];
    float g[16];
    int act[16];
};

// The critic MLP over the 16-row tile starting at row0 of timestep t: relu(fc1), relu(fc2) into L.h1 / L.h2, q
// [row][a] into L.q. One wave.
__device__ void critic_forward_tile(const ComaDev& c, const float* __restrict__ P, int t, int row0, CriticLds& L,
                                    int lane) {
    const int col = lane & 15, g = lane >> 4;
    const int R = c.B * c.N;
    const int row = row0 + col;
    const bool valid = row < R;
    const int b = valid ? row / c.N : 0, n = valid ? row % c.N : 0;
    const int slot = coma_slot(c.bt, b);
    const ComaOffsets o = coma_offsets(c.D, c.A);
    floatx4 acc[8];
    dense16<8>(acc, P + o.w1, c.D, 1, P + o.b1, CH, c.D, lane,
               [&](int k) { return valid ? critic_x(c, slot, t, n, k) : 0.f; });
#pragma unroll
    for (int ot = 0; ot < 8; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) L.h1[col * CLD + 16 * ot + 4 * g + r] = fmaxf(acc[ot][r], 0.f);
    __syncthreads();
    dense16<8>(acc, P + o.w2, CH, 1, P + o.b2, CH, CH, lane, [&](int k) { return L.h1[col * CLD + k]; });
#pragma unroll
    for (int ot = 0; ot < 8; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) L.h2[col * CLD + 16 * ot + 4 * g + r] = fmaxf(acc[ot][r], 0.f);
    __syncthreads();
    floatx4 qa[6];
    dense16<6>(qa, P + o.w3, CH, 1, P + o.b3, c.A, CH, lane, [&](int k) { return L.h2[col * CLD + k]; });
#pragma unroll
    for (int at = 0; at < 6; ++at)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = 16 * at + 4 * g + r;
            if (a < c.A) L.q[col * (CMAXA + 1) + a] = qa[at][r];
        }
    __syncthreads();
}

// Target critic over all timesteps: grid (row tiles, T); tq[b][t][n] = Q_target(b, t, n)[action].
__global__ void __launch_bounds__(64) coma_target_kernel(ComaDev c, const float* __restrict__ P) {
    __shared__ CriticLds L;
    const int lane = threadIdx.x, t = blockIdx.y, row0 = blockIdx.x * 16;
    critic_forward_tile(c, P, t, row0, L, lane);
    const int row = row0 + lane;
    if (lane < 16 && row < c.B * c.N) {
        const int b = row / c.N, n = row % c.N;
        const int64_t st = (int64_t)coma_slot(c.bt, b) * c.bt.T1 + t;
        int a = (int)c.bt.actions[st * c.N + n];
        a = a < 0 ? 0 : (a >= c.A ? c.A - 1 : a);
        c.tq[((int64_t)b * c.T + t) * c.N + n] = L.q[lane * (CMAXA + 1) + a];
    }
}

// Masks, per-step mask sums and the TD(lambda) targets (build_td_lambda_targets); zeroes the stats. One workgroup.
__global__ void __launch_bounds__(256) coma_td_lambda_kernel(ComaDev c, float lam_gamma, float one_lam_gamma) {
    const int tid = threadIdx.x, Tm = c.T - 1;
    if (tid < 6) c.stats[tid] = 0.f;
    for (int i = tid; i < c.B * Tm; i += 256) {
        const int b = i / Tm, t = i % Tm;
        const int64_t st = (int64_t)coma_slot(c.bt, b) * c.bt.T1 + t;
        float m = (float)c.bt.filled[st];
        if (t > 0) m = m * (1.f - (float)c.bt.terminated[st - 1]);
        c.masks[i] = m;
    }
    __syncthreads();
    for (int t = tid; t < Tm; t += 256) {
        float s = 0.f;
        for (int b = 0; b < c.B; ++b) s += c.masks[b * Tm + t];
        c.masksum[t] = s;
    }
    for (int i = tid; i < c.B * c.N; i += 256) {
        const int b = i / c.N, n = i % c.N;
        const int64_t s0 = (int64_t)coma_slot(c.bt, b) * c.bt.T1;
        float term_sum = 0.f;
        for (int t = 0; t < Tm; ++t) term_sum += (float)c.bt.terminated[s0 + t];
        float ret = c.tq[((int64_t)b * c.T + Tm) * c.N + n] * (1.f - term_sum);
        for (int t = Tm - 1; t >= 0; --t) {
            const float term = (float)c.bt.terminated[s0 + t];
            const float nxt = c.tq[((int64_t)b * c.T + t + 1) * c.N + n];
            ret = lam_gamma * ret + c.masks[b * Tm + t] * (c.bt.reward[s0 + t] + one_lam_gamma * nxt * (1.f - term));
            c.targets[((int64_t)b * Tm + t) * c.N + n] = ret;
        }
    }
}

// One critic step, launch 1 of 3: forward at t with the live parameters, q_vals[:, t], the TD error and the deltas
// of the three layers. One wave per 16-row tile.
__global__ void __launch_bounds__(64) coma_step_forward_kernel(ComaDev c, const float* __restrict__ P, int t) {
    __shared__ CriticLds L;
    const int lane = threadIdx.x, row0 = blockIdx.x * 16;
    const int col = lane & 15, g = lane >> 4;
    const int R = c.B * c.N, Tm = c.T - 1;
    const float msum = c.masksum[t];
    if (msum == 0.f) {  // the whole step is skipped: q_vals[:, t] stays zero
        for (int i = lane; i < 16 * c.A; i += 64) {
            const int row = row0 + i / c.A, a = i % c.A;
            if (row < R) c.q_vals[(((int64_t)(row / c.N) * Tm + t) * c.N + row % c.N) * c.A + a] = 0.f;
        }
        return;
    }
    critic_forward_tile(c, P, t, row0, L, lane);
    const ComaOffsets o = coma_offsets(c.D, c.A);
    for (int i = lane; i < 16 * c.A; i += 64) {
        const int rr = i / c.A, a = i % c.A, row = row0 + rr;
        if (row < R)
            c.q_vals[(((int64_t)(row / c.N) * Tm + t) * c.N + row % c.N) * c.A + a] = L.q[rr * (CMAXA + 1) + a];
    }
    if (lane < 16) {
        const int row = row0 + lane;
        float gq = 0.f;
        int a = 0;
        if (row < R) {
            const int b = row / c.N, n = row % c.N;
            const int64_t st = (int64_t)coma_slot(c.bt, b) * c.bt.T1 + t;
            a = (int)c.bt.actions[st * c.N + n];
            a = a < 0 ? 0 : (a >= c.A ? c.A - 1 : a);
            const float qt = L.q[lane * (CMAXA + 1) + a];
            const float tgt = c.targets[((int64_t)b * Tm + t) * c.N + n];
            const float mk = c.masks[b * Tm + t];
            const float mtd = (qt - tgt) * mk;
            float* rs = c.rowstats + (int64_t)row * 4;
            rs[0] = mtd * mtd;
            rs[1] = fabsf(mtd);
            rs[2] = qt * mk;
            rs[3] = tgt * mk;
            gq = 2.f * mtd * mk / ((float)c.N * msum);
            c.d3[row] = gq;
        }
        L.g[lane] = gq;
        L.act[lane] = a;
    }
    __syncthreads();
    // delta2 = (fc3.weight[a] * gq) where relu(fc2) > 0
    for (int i = lane; i < 16 * CH; i += 64) {
        const int rr = i / CH, j = i % CH, row = row0 + rr;
        const float v = L.h2[rr * CLD + j] > 0.f ? L.g[rr] * P[o.w3 + (int64_t)L.act[rr] * CH + j] : 0.f;
        L.d2[rr * CLD + j] = v;
        if (row < R) {
            c.d2[(int64_t)row * CH + j] = v;
            c.h1[(int64_t)row * CH + j] = L.h1[rr * CLD + j];
            c.h2[(int64_t)row * CH + j] = L.h2[rr * CLD + j];
        }
    }
    __syncthreads();
    // delta1 = (fc2.weight^T delta2) where relu(fc1) > 0
    floatx4 acc[8];
    dense16<8>(acc, P + o.w2, 1, CH, nullptr, CH, CH, lane, [&](int k) { return L.d2[col * CLD + k]; });
    const int row = row0 + col;
    if (row < R) {
#pragma unroll
        for (int ot = 0; ot < 8; ++ot)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * ot + 4 * g + r;
                c.d1[(int64_t)row * CH + i] = L.h1[col * CLD + i] > 0.f ? acc[ot][r] : 0.f;
            }
    }
}

// Launch 2 of 3: one thread per parameter sums its gradient over the rows in ascending order; each workgroup leaves
// the sum of its squared gradients (fixed tree) for the norm.
__global__ void __launch_bounds__(256) coma_step_grads_kernel(ComaDev c, float* __restrict__ grads, int t) {
    __shared__ float red[256];
    if (c.masksum[t] == 0.f) return;
    const ComaOffsets o = coma_offsets(c.D, c.A);
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int R = c.B * c.N;
    float gsum = 0.f;
    int64_t pidx = -1;
    if (e < o.b1) {  // fc1.weight: feature fastest over the threads (delta1 rows are read coalesced)
        const int f = (int)(e % CH), k = (int)(e / CH);
        pidx = o.w1 + (int64_t)f * c.D + k;
        for (int r = 0; r < R; ++r) {
            const int b = r / c.N, n = r % c.N;
            gsum += c.d1[(int64_t)r * CH + f] * critic_x(c, coma_slot(c.bt, b), t, n, k);
        }
    } else if (e < o.w2) {
        const int f = (int)(e - o.b1);
        pidx = e;
        for (int r = 0; r < R; ++r) gsum += c.d1[(int64_t)r * CH + f];
    } else if (e < o.b2) {
        const int64_t i = e - o.w2;
        const int f = (int)(i % CH), k = (int)(i / CH);
        pidx = o.w2 + (int64_t)f * CH + k;
        for (int r = 0; r < R; ++r) gsum += c.d2[(int64_t)r * CH + f] * c.h1[(int64_t)r * CH + k];
    } else if (e < o.w3) {
        const int f = (int)(e - o.b2);
        pidx = e;
        for (int r = 0; r < R; ++r) gsum += c.d2[(int64_t)r * CH + f];
    } else if (e < o.total) {
        const bool is_w = e < o.b3;
        const int64_t i = e - (is_w ? o.w3 : o.b3);
        const int a = is_w ? (int)(i / CH) : (int)i, k = is_w ? (int)(i % CH) : 0;
        pidx = e;
        for (int r = 0; r < R; ++r) {
            const int b = r / c.N, n = r % c.N;
            const int64_t st = (int64_t)coma_slot(c.bt, b) * c.bt.T1 + t;
            int ar = (int)c.bt.actions[st * c.N + n];
            ar = ar < 0 ? 0 : (ar >= c.A ? c.A - 1 : ar);
            if (ar == a) gsum += is_w ? c.d3[r] * c.h2[(int64_t)r * CH + k] : c.d3[r];
        }
    }
    if (pidx >= 0) grads[pidx] = gsum;
    const float sq = block_sum(gsum * gsum, red);
    if (threadIdx.x == 0) c.partial[blockIdx.x] = sq;
}

// Launch 3 of 3: clip_grad_norm_ and RMSprop over the workgroup's parameters; workgroup 0 adds the step's stats.
__global__ void __launch_bounds__(256) coma_step_update_kernel(ComaDev c, float* __restrict__ params,
                                                              float* __restrict__ grads, float* __restrict__ sq_avg,
                                                              int64_t n_params, int n_partial, float lr, float alpha,
                                                              float one_minus_alpha, float eps, float clip, int t) {
    __shared__ float red[256];
    const float msum = c.masksum[t];
    if (msum == 0.f) return;
    float s = 0.f;
    for (int i = threadIdx.x; i < n_partial; i += 256) s += c.partial[i];
    const float norm = sqrtf(block_sum(s, red));
    const float coef = fminf(clip / (norm + 1e-6f), 1.f);
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n_params) {
        const float g = grads[e] * coef;
        grads[e] = g;
        const float sq = sq_avg[e] * alpha + one_minus_alpha * (g * g);
        sq_avg[e] = sq;
        params[e] = params[e] - lr * (g / (sqrtf(sq) + eps));
    }
    if (blockIdx.x != 0) return;
    const int R = c.B * c.N;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = threadIdx.x; r < R; r += 256)
        for (int j = 0; j < 4; ++j) v[j] += c.rowstats[(int64_t)r * 4 + j];
    float tot[4];
    for (int j = 0; j < 4; ++j) tot[j] = block_sum(v[j], red);
    if (threadIdx.x == 0) {
        const float den = (float)c.N * msum;
        c.stats[0] += tot[0] / den;
        c.stats[1] += norm;
        c.stats[2] += tot[1] / den;
        c.stats[3] += tot[2] / den;
        c.stats[4] += tot[3] / den;
        c.stats[5] += 1.f;
        c.counters[0] += 1;
    }
}

__global__ void coma_target_copy_kernel(const float* __restrict__ params, float* __restrict__ target, int64_t n,
                                        const int64_t* __restrict__ counters, int interval) {
    if (counters[0] - counters[1] < (int64_t)interval) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) target[i] = params[i];
}
__global__ void coma_target_mark_kernel(int64_t* __restrict__ counters, int interval) {
    if (counters[0] - counters[1] >= (int64_t)interval) counters[1] = counters[0];
}

int check_coma_cfg(const MlgComaCfg* c) {
    MLG_REQUIRE(c != nullptr, "null coma cfg");
    MLG_REQUIRE(c->hidden == CH, "coma critic hidden=%d unsupported (128)", c->hidden);
    MLG_REQUIRE(c->N >= 1 && c->N <= 32, "coma critic n_agents N=%d unsupported (1..32)", c->N);
    MLG_REQUIRE(c->A >= 1 && c->A <= CMAXA, "coma critic n_actions A=%d unsupported (1..96)", c->A);
    MLG_REQUIRE(c->B >= 1 && c->B <= 4096, "coma critic batch B=%d unsupported (1..4096)", c->B);
    MLG_REQUIRE(c->T >= 2 && c->T <= 65535, "coma critic T=%d unsupported (2..65535)", c->T);
    MLG_REQUIRE(c->d_obs >= 1 && c->S >= 1, "coma critic d_obs=%d / S=%d invalid", c->d_obs, c->S);
    return 0;
}

inline int coma_D(const MlgComaCfg* c) { return c->S + c->d_obs + 2 * c->N * c->A + c->N; }
inline int64_t al4(int64_t n) { return (n + 3) & ~(int64_t)3; }

}  // namespace

extern "C" int mlg_policy_probs(const float* logits, const int32_t* avail, int32_t R, int32_t A, float epsilon,
                                int32_t mask_before_softmax, int32_t test_mode, float* probs, void* stream) {
    MLG_REQUIRE(logits && avail && probs && R >= 0 && A >= 1, "policy_probs: bad arguments");
    if (R == 0) return 0;
    hipLaunchKernelGGL(policy_probs_kernel<false>, dim3((R + 63) / 64), dim3(64), 0, (hipStream_t)stream, logits, avail,
                       (const float*)nullptr, R, A, epsilon, mask_before_softmax, test_mode, probs);
    return mlg::check_launch("policy_probs_kernel");
}

extern "C" int mlg_policy_probs_backward(const float* logits, const int32_t* avail, const float* g_probs, int32_t R,
                                         int32_t A, float epsilon, int32_t mask_before_softmax, int32_t test_mode,
                                         float* d_logits, void* stream) {
    MLG_REQUIRE(logits && avail && g_probs && d_logits && R >= 0 && A >= 1, "policy_probs_backward: bad arguments");
    if (R == 0) return 0;
    hipLaunchKernelGGL(policy_probs_kernel<true>, dim3((R + 63) / 64), dim3(64), 0, (hipStream_t)stream, logits, avail,
                       g_probs, R, A, epsilon, mask_before_softmax, test_mode, d_logits);
    return mlg::check_launch("policy_probs_backward_kernel");
}

extern "C" int mlg_select_multinomial(const float* probs, const int32_t* avail, int32_t R, int32_t A,
                                      int32_t n_agents, const uint64_t* keys, const uint32_t* episodes, int32_t t,
                                      int32_t greedy, int64_t* actions, void* stream) {
    MLG_REQUIRE(probs && avail && actions && R >= 0 && A >= 1 && n_agents >= 1, "select_multinomial: bad arguments");
    MLG_REQUIRE(greedy || keys, "select_multinomial: sampling needs rng keys");
    if (R == 0) return 0;
    hipLaunchKernelGGL(select_multinomial_kernel, dim3((R + 63) / 64), dim3(64), 0, (hipStream_t)stream, probs, avail, R,
                       A, n_agents, keys, episodes, t, greedy, actions);
    return mlg::check_launch("select_multinomial_kernel");
}

extern "C" int mlg_coma_policy_loss(const float* pi, const int32_t* avail, const int64_t* actions, const float* q_vals,
                                    const float* mask, int32_t rows, int32_t N, int32_t A, float* out, float* d_pi,
                                    void* stream) {
    MLG_REQUIRE(pi && avail && actions && q_vals && mask && out && d_pi, "coma_policy_loss: null pointer");
    MLG_REQUIRE(rows >= 0 && N >= 1 && A >= 1 && (int64_t)rows * N < (1 << 30), "coma_policy_loss: bad sizes");
    hipLaunchKernelGGL(coma_policy_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, pi, avail, actions, q_vals,
                       mask, rows, N, A, out, d_pi);
    return mlg::check_launch("coma_policy_loss_kernel");
}

extern "C" int64_t mlg_coma_param_count(const MlgComaCfg* c) {
    if (check_coma_cfg(c)) return -1;
    return coma_offsets(coma_D(c), c->A).total;
}

extern "C" int64_t mlg_coma_workspace_floats(const MlgComaCfg* c) {
    if (check_coma_cfg(c)) return -1;
    const int64_t R = (int64_t)c->B * c->N, Tm = c->T - 1;
    const int64_t n_blocks = (coma_offsets(coma_D(c), c->A).total + 255) / 256;
    return al4(R * c->T) + al4(c->B * Tm) + al4(Tm) + 4 * al4(R * CH) + al4(R) + al4(R * 4) + al4(n_blocks);
}

extern "C" int mlg_coma_critic_train(const MlgComaCfg* cfg, const MlgComaBufs* b, void* stream) {
    if (check_coma_cfg(cfg)) return 1;
    MLG_REQUIRE(b && b->params && b->grads && b->square_avg && b->target_params && b->workspace && b->q_vals &&
                    b->targets && b->stats && b->counters,
                "coma_critic_train: null buffer");
    const MlgBatch& bt = b->batch;
    MLG_REQUIRE(bt.state && bt.obs && bt.actions && bt.reward && bt.terminated && bt.actions_onehot && bt.filled,
                "coma_critic_train: the batch lacks a key");
    MLG_REQUIRE(bt.B == cfg->B && bt.T1 >= cfg->T, "coma_critic_train: batch B=%d T1=%d do not hold cfg B=%d T=%d", bt.B,
                bt.T1, cfg->B, cfg->T);
    hipStream_t s = (hipStream_t)stream;
    ComaDev c{};
    c.bt = bt;
    c.B = cfg->B; c.T = cfg->T; c.N = cfg->N; c.A = cfg->A; c.DO = cfg->d_obs; c.S = cfg->S;
    c.D = coma_D(cfg);
    const int64_t R = (int64_t)c.B * c.N, Tm = c.T - 1;
    const ComaOffsets o = coma_offsets(c.D, c.A);
    const int n_blocks = (int)((o.total + 255) / 256);
    float* w = b->workspace;
    c.tq = w; w += al4(R * c.T);
    c.masks = w; w += al4(c.B * Tm);
    c.masksum = w; w += al4(Tm);
    c.h1 = w; w += al4(R * CH);
    c.h2 = w; w += al4(R * CH);
    c.d1 = w; w += al4(R * CH);
    c.d2 = w; w += al4(R * CH);
    c.d3 = w; w += al4(R);
    c.rowstats = w; w += al4(R * 4);
    c.partial = w;
    c.q_vals = b->q_vals;
    c.targets = b->targets;
    c.stats = b->stats;
    c.counters = b->counters;
    const int tiles = (int)((R + 15) / 16);
    hipLaunchKernelGGL(coma_target_kernel, dim3(tiles, c.T), dim3(64), 0, s, c, b->target_params);
    if (mlg::check_launch("coma_target_kernel")) return 1;
    const float lam_gamma = (float)(cfg->td_lambda * cfg->gamma);
    const float one_lam_gamma = (float)((1.0 - cfg->td_lambda) * cfg->gamma);
    hipLaunchKernelGGL(coma_td_lambda_kernel, dim3(1), dim3(256), 0, s, c, lam_gamma, one_lam_gamma);
    if (mlg::check_launch("coma_td_lambda_kernel")) return 1;
    for (int t = c.T - 2; t >= 0; --t) {
        hipLaunchKernelGGL(coma_step_forward_kernel, dim3(tiles), dim3(64), 0, s, c, (const float*)b->params, t);
        hipLaunchKernelGGL(coma_step_grads_kernel, dim3(n_blocks), dim3(256), 0, s, c, b->grads, t);
        hipLaunchKernelGGL(coma_step_update_kernel, dim3(n_blocks), dim3(256), 0, s, c, b->params, b->grads,
                           b->square_avg, o.total, n_blocks, cfg->lr, (float)cfg->optim_alpha,
                           (float)(1.0 - cfg->optim_alpha), cfg->optim_eps, cfg->grad_norm_clip, t);
        if (mlg::check_launch("coma critic step")) return 1;
    }
    return 0;
}

extern "C" int mlg_coma_target_update(const float* params, float* target_params, int64_t n, int64_t* counters,
                                      int32_t interval, void* stream) {
    MLG_REQUIRE(params && target_params && counters && n >= 0 && interval >= 1, "coma_target_update: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (n > 0)
        hipLaunchKernelGGL(coma_target_copy_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, params,
                           target_params, n, (const int64_t*)counters, interval);
    hipLaunchKernelGGL(coma_target_mark_kernel, dim3(1), dim3(1), 0, s, counters, interval);
    return mlg::check_launch("coma_target_update");
}
