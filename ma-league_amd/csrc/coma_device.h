// coma_device.h -- what the COMA kernels share (coma.hip, rollout_policy.hip, crossplay.hip).
#pragma once
#include "agent_device.h"
#include "mlg_device.h"

// Counter-RNG purpose of the multinomial policy draw. 1-3 are mlg_device.h's (spawn, epsilon coin,
// random action), 4 the entity env's team draw (refil_device.h).
enum { MLG_PURPOSE_POLICY = 5 };

namespace {

// Multinomial policy pick for the lane's row (mlg_rollout_policy: MultiAgentController._softmax,
// multi_agent_controller.py:78-99, then MultinomialActionSelector.select, action_selectors.py:11-32, with the draw rule
// of mlg_select_multinomial). qt[at][r] is the logit of action 16 at + 4 g + r; the four lanes col + 16 g of a row
// share the work and every one returns the action. Sums add each lane's four entries first, then the lanes in
// ascending g, then the tiles in ascending order. All 64 lanes must be active; av == nullptr: every action available.
constexpr int RO_MAXAT = 5;  // n_actions = 5 + U <= 69 fits five 16-wide tiles
__device__ __forceinline__ int ro_policy_select(floatx4 (&qt)[RO_MAXAT], int n_at, const int32_t* av, int A, int lane,
                                                float eps, bool mask, bool test_mode, bool greedy, float u) {
    const int g = lane >> 4;
    auto xor_f = [](float v, int m) { return __shfl_xor(v, m); };
    unsigned ok = 0u;  // bit 4 at + r: the action is in range and available
    float mx = -INFINITY;
#pragma unroll
    for (int at = 0; at < RO_MAXAT; ++at)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = at * 16 + 4 * g + r;
            const bool in = at < n_at && a < A;
            const bool on = in && (av == nullptr || av[a] != 0);
            ok |= (unsigned)on << (4 * at + r);
            const float x = in ? ((mask && !on) ? -1e10f : qt[at][r]) : -INFINITY;
            qt[at][r] = x;
            mx = fmaxf(mx, x);
        }
    mx = fmaxf(mx, xor_f(mx, 16));
    mx = fmaxf(mx, xor_f(mx, 32));
    int K = __popc(ok);
    K += __shfl_xor(K, 16);
    K += __shfl_xor(K, 32);
    float s = 0.f;
#pragma unroll
    for (int at = 0; at < RO_MAXAT; ++at)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            qt[at][r] = expf(qt[at][r] - mx);  // exp(-inf) = 0 for the entries out of range
            s += qt[at][r];
        }
    s += xor_f(s, 16);
    s += xor_f(s, 32);
    const float keep = 1.f - eps, floor_p = eps / (float)(mask ? K : A);
    // m_k: the probability where available, else 0
#pragma unroll
    for (int at = 0; at < RO_MAXAT; ++at)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = qt[at][r] / s;
            qt[at][r] = ((ok >> (4 * at + r)) & 1u) ? (test_mode ? p : keep * p + floor_p) : 0.f;
        }
    if (greedy) {
        ArgmaxState as{-INFINITY, 1 << 30};
#pragma unroll
        for (int at = 0; at < RO_MAXAT; ++at)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a = at * 16 + 4 * g + r;
                const float v = ((ok >> (4 * at + r)) & 1u) ? qt[at][r] : -INFINITY;
                if (a < A && amax_better(v, a, as.bv, as.bi)) { as.bv = v; as.bi = a; }
            }
        const int act = argmax_reduce(as);
        return act < A ? act : 0;
    }
    const int col = lane & 15;
    float total = 0.f;
#pragma unroll
    for (int at = 0; at < RO_MAXAT; ++at) {
        const float ls = ((qt[at][0] + qt[at][1]) + qt[at][2]) + qt[at][3];
        total = (((total + __shfl(ls, col)) + __shfl(ls, col + 16)) + __shfl(ls, col + 32)) + __shfl(ls, col + 48);
    }
    const float thr = u * total;
    float run = 0.f;
    int pick = 1 << 30, last = -1;
#pragma unroll
    for (int at = 0; at < RO_MAXAT; ++at) {
        const float ls = ((qt[at][0] + qt[at][1]) + qt[at][2]) + qt[at][3];
        const float s0 = __shfl(ls, col), s1 = __shfl(ls, col + 16), s2 = __shfl(ls, col + 32),
                    s3 = __shfl(ls, col + 48);
        float c = run;
        if (g > 0) c += s0;
        if (g > 1) c += s1;
        if (g > 2) c += s2;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (!((ok >> (4 * at + r)) & 1u)) continue;
            const int a = at * 16 + 4 * g + r;
            c += qt[at][r];
            last = a;
            if (pick == (1 << 30) && c > thr) pick = a;
        }
        run = (((run + s0) + s1) + s2) + s3;
    }
    pick = min(pick, __shfl_xor(pick, 16));
    pick = min(pick, __shfl_xor(pick, 32));
    last = max(last, __shfl_xor(last, 16));
    last = max(last, __shfl_xor(last, 32));
    return pick != (1 << 30) ? pick : (last >= 0 ? last : 0);
}

}  // namespace
