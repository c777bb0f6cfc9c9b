// agent_ff_device.h -- the feed-forward agent (fc1 -> ReLU -> fc2; DQNAgentNetwork.forward,
// src/marl/modules/agents/dqn_agent.py:9-37) on the DRQN cell's building blocks: agent_fc1 and agent_q_tile of
// agent_device.h run unchanged over a weight view whose GRU offsets are never read.
//
// Packed weight block (floats; every offset 16-byte aligned; H % 16 == 0), the DRQN block's paddings and transposes
// without the GRU blocks and the split-bf16 images:
//   w1d [H][Dip], w1o [H][Dob], w1a [A][H] (iff obs_last_action), w1n [N][H] (iff obs_agent_id), b1 [H],
//   w2 [Ap][H], b2 [Ap]
#pragma once
#include "agent_device.h"

// The block's layout as an AgentLayout (what agent_fc1 / global_view take): the GRU and split-image offsets stay 0.
__host__ __device__ constexpr AgentLayout make_ff_layout(const MlgAgentDims& d) {
    AgentLayout L{};
    L.H = d.hidden;
    L.A = d.n_actions;
    L.Ap = (d.n_actions + 15) / 16 * 16;
    L.N = d.n_agents;
    L.d_obs = d.d_obs;
    L.Dob = (d.d_obs + 15) / 16 * 16;
    L.d_in = d.d_in;
    L.Dip = (d.d_in + 15) / 16 * 16;
    L.last_action = d.obs_last_action;
    L.agent_id = d.obs_agent_id;
    int64_t o = 0;
    L.w1d = o; o += (int64_t)L.H * L.Dip;
    L.w1o = o; o += (int64_t)L.H * L.Dob;
    L.w1a = o; o += L.last_action ? (int64_t)L.A * L.H : 0;
    L.w1n = o; o += L.agent_id ? (int64_t)L.N * L.H : 0;
    L.b1 = o; o += L.H;
    L.w2 = o; o += (int64_t)L.Ap * L.H;
    L.b2 = o; o += L.Ap;
    L.total = mlg_align4(o);
    return L;
}

// Packed float i of the block from the canonical nn.Module tensors.
__device__ __forceinline__ float pack_ff_elem(const AgentLayout& L, const MlgFFParams& p, int64_t i) {
    const int H = L.H;
    float v = 0.f;
    if (i < L.w1o) {  // dense fc1 [H][Dip]
        const int64_t r = i / L.Dip, c = i % L.Dip;
        v = c < L.d_in ? p.fc1_w[r * L.d_in + c] : 0.f;
    } else if (i < L.w1a) {  // obs columns [H][Dob]
        const int64_t k = i - L.w1o, r = k / L.Dob, c = k % L.Dob;
        v = c < L.d_obs ? p.fc1_w[r * L.d_in + c] : 0.f;
    } else if (i < L.w1n) {  // last-action columns transposed [A][H]
        const int64_t k = i - L.w1a, a = k / H, r = k % H;
        v = p.fc1_w[r * L.d_in + L.d_obs + a];
    } else if (i < L.b1) {  // agent-id columns transposed [N][H]
        const int64_t k = i - L.w1n, n = k / H, r = k % H;
        v = p.fc1_w[r * L.d_in + L.d_obs + (L.last_action ? L.A : 0) + n];
    } else if (i < L.w2) {
        v = p.fc1_b[i - L.b1];
    } else if (i < L.b2) {
        const int64_t k = i - L.w2, r = k / H, c = k % H;
        v = r < L.A ? p.fc2_w[r * H + c] : 0.f;
    } else if (i < L.b2 + L.Ap) {
        const int64_t k = i - L.b2;
        v = k < L.A ? p.fc2_b[k] : 0.f;
    }
    return v;
}

// LDS image of the rollout kernel (no dense w1d): w1o, w1a, w1n, b1, w2, b2 with the DRQN image's padded row strides.
__host__ __device__ inline LdsWeights make_ff_lds_weights(const AgentLayout& L) {
    LdsWeights w{};
    w.ldo = L.Dob + 4;
    w.ldh = L.H + 4;
    int64_t o = 0;
    w.w1o = o; o += (int64_t)L.H * w.ldo;
    w.w1a = o; o += L.last_action ? (int64_t)L.A * w.ldh : 0;
    w.w1n = o; o += L.agent_id ? (int64_t)L.N * w.ldh : 0;
    w.b1 = o; o += L.H;
    w.w2 = o; o += (int64_t)L.Ap * w.ldh;
    w.b2 = o; o += L.Ap;
    w.total = mlg_align4(o);
    return w;
}

// Cooperative copy packed (global) -> padded LDS image (whole workgroup; caller syncs).
__device__ inline void load_ff_weights_to_lds(const float* __restrict__ P, const AgentLayout& L, const LdsWeights& w,
                                              float* lds) {
    const int H = L.H;
    auto rows = [&](int64_t src, int64_t dst, int nrows, int ncols, int ld) {
        for (int i = threadIdx.x; i < nrows * ncols; i += blockDim.x) {
            const int r = i / ncols, c = i % ncols;
            lds[dst + (int64_t)r * ld + c] = P[src + (int64_t)r * ncols + c];
        }
    };
    rows(L.w1o, w.w1o, H, L.Dob, w.ldo);
    if (L.last_action) rows(L.w1a, w.w1a, L.A, H, w.ldh);
    if (L.agent_id) rows(L.w1n, w.w1n, L.N, H, w.ldh);
    rows(L.b1, w.b1, 1, H, H);
    rows(L.w2, w.w2, L.Ap, H, w.ldh);
    rows(L.b2, w.b2, 1, L.Ap, L.Ap);
}

// fc1 + ReLU for one tile -> x (HC chunks, D layout).
template <int H, bool DENSE>
__device__ __forceinline__ void ff_hidden(const WView& W, const AgentLayout& L, const RowIn& in, floatx4 (&x)[H / 16],
                                          int lane) {
    agent_fc1<H, DENSE>(W, L, in, x, lane);
#pragma unroll
    for (int mt = 0; mt < H / 16; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) x[mt][r] = fmaxf(x[mt][r], 0.f);
}
