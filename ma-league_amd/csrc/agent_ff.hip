// agent_ff.hip -- the feed-forward agent's entry points: weight packing, forward over arbitrary rows, BasicMAC.forward
// from an EpisodeBatch, and the backward of one forward call (the kernel behind the autograd formula of
// torch.ops.maleague.dqn_forward). The forward is agent.hip's agent_forward_kernel without the GRU cell; the backward
// follows agent_grad.hip: a row pass that writes activations and deltas to the workspace, then the weight gradients
// as block jobs of wgrad_device.h (one wgrad launch, one fixed-order reduce: deterministic, no float atomics).
#include "agent_ff_device.h"
#include "mlg_host.h"
#include "wgrad_device.h"

int check_agent_dims(const MlgAgentDims* d);  // agent.hip

namespace {

using GJobs = mlg::BJobsT<16>;

// One thread per packed float.
__global__ void pack_ff_kernel(AgentLayout L, MlgFFParams p, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.total) return;
    out[i] = pack_ff_elem(L, p, i);
}

// q = fc2(relu(fc1(x))) over R rows; one wave per 16-row tile. DENSE: inputs[R][d_in]. MAC mode: rows = (b, n) of an
// EpisodeBatch at time t, inputs built from obs / actions_onehot(t-1) / id (agent_forward_kernel's row addressing).
template <int H, bool DENSE>
__global__ void __launch_bounds__(256) ff_forward_kernel(AgentLayout L, const float* __restrict__ P,
                                                        const float* __restrict__ inputs, MlgBatch bt, int t,
                                                        float* __restrict__ q, int R) {
    constexpr int HC = H / 16;
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (tile * 16 >= R) return;  // whole wave exits together
    const int col = lane & 15, g = lane >> 4;
    const int row = tile * 16 + col;
    const bool valid = row < R;
    RowIn in;
    in.prev_action = -1;
    if (DENSE) {
        in.x = valid ? inputs + (int64_t)row * L.d_in : nullptr;
        in.onehot = nullptr;
        in.agent = 0;
    } else {
        const int N = L.N, b = row / N, n = row % N;
        const int64_t off = valid ? ((bt.rows ? (int64_t)bt.rows[b] : (int64_t)b) * bt.T1 + t) * N + n : 0;
        in.x = valid ? bt.obs + off * L.d_obs : nullptr;
        in.onehot = (valid && t > 0) ? bt.actions_onehot + (off - N) * L.A : nullptr;
        in.agent = valid ? n : 0;
    }
    const WView W = global_view(P, L);
    floatx4 x[HC];
    ff_hidden<H, DENSE>(W, L, in, x, lane);
    for (int at = 0; at < L.Ap / 16; ++at) {
        const floatx4 qt = agent_q_tile<H>(W, x, at, lane);
        if (!valid) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = at * 16 + 4 * g + r;
            if (a < L.A) q[(int64_t)row * L.A + a] = qt[r];
        }
    }
}

// workspace rows (all [R][...], written by the row pass, read by the wgrad jobs)
struct FFGradWs {
    float *x, *gq, *dx;
};

// One wave per 16-row tile, f32 MFMA in the forward's orientation. Forward recomputed, then
//   dh = W2^T gq;  dx = dh [x > 0];  d_inputs = W1^T dx
// The deltas go to the workspace in [row][feature] order; a lane reads back nothing, so the pass needs no barrier.
template <int H>
__global__ void __launch_bounds__(256) ff_backward_kernel(AgentLayout L, const float* __restrict__ P,
                                                         const float* __restrict__ inputs,
                                                         const float* __restrict__ gq, FFGradWs w,
                                                         float* __restrict__ d_inputs, int R) {
    constexpr int HC = H / 16;
    const int lane = threadIdx.x & 63;
    const int tile = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (tile * 16 >= R) return;  // whole wave exits together
    const int col = lane & 15, g = lane >> 4;
    const int row = tile * 16 + col;
    const bool valid = row < R;
    const int64_t rh = (int64_t)row * H;
    const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
    RowIn in;
    in.x = valid ? inputs + (int64_t)row * L.d_in : nullptr;
    in.onehot = nullptr;
    in.prev_action = -1;
    in.agent = 0;
    const WView W = global_view(P, L);
    floatx4 x[HC];
    ff_hidden<H, true>(W, L, in, x, lane);
    const float* gqr = (valid && gq) ? gq + (int64_t)row * L.A : nullptr;
    if (valid)
        for (int a = g; a < L.A; a += 4) w.gq[(int64_t)row * L.A + a] = gqr ? gqr[a] : 0.f;
    floatx4 dx[HC];
#pragma unroll
    for (int mt = 0; mt < HC; ++mt) {
        // dh = W2^T gq (fc2 rows past A are zero in the packed block)
        floatx4 dh = zero;
        if (gq)
            for (int at = 0; at < L.Ap / 16; ++at)
                dh = mfma_chunk(ld_col4(P + W.w2, at * 16 + 4 * g, W.ldh, mt * 16 + col),
                                load_chunk(gqr, at * 16 + 4 * g, L.A), dh);
#pragma unroll
        for (int r = 0; r < 4; ++r) dx[mt][r] = x[mt][r] > 0.f ? dh[r] : 0.f;
        if (valid) {
            st4(w.x + rh + mt * 16 + 4 * g, x[mt]);
            st4(w.dx + rh + mt * 16 + 4 * g, dx[mt]);
        }
    }
    // ---- d_inputs = W1^T dx (dense fc1 [H][Dip], columns past d_in zero) ----
    if (!d_inputs) return;
    for (int jt = 0; jt < L.Dip / 16; ++jt) {
        floatx4 acc = zero;
#pragma unroll
        for (int kc = 0; kc < HC; ++kc)
            acc = mfma_chunk(ld_col4(P + W.w1d, kc * 16 + 4 * g, W.ldd, jt * 16 + col), dx[kc], acc);
        if (!valid) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = jt * 16 + 4 * g + r;
            if (j < L.d_in) d_inputs[(int64_t)row * L.d_in + j] = acc[r];
        }
    }
}

struct FFGradPlan {
    int64_t x, gq, dx, slab, nrm, total, n_params;
    int n_tasks;
    int64_t n_red;
    GJobs J;
};

// workspace offsets and the job table; ws == nullptr: sizes only
FFGradPlan ff_grad_plan(const MlgAgentDims& d, int R, float* ws, const float* inputs, float* dparams) {
    FFGradPlan p{};
    const int H = d.hidden, A = d.n_actions, Din = d.d_in;
    int64_t o = 0;
    auto take = [&](int64_t n) {
        const int64_t at = o;
        o += mlg_align4(n);
        return at;
    };
    p.x = take((int64_t)R * H);
    p.gq = take((int64_t)R * A);
    p.dx = take((int64_t)R * H);
    p.slab = o;
    // dparams in named_parameters() order: fc1.weight, fc1.bias, fc2.weight, fc2.bias
    const int64_t fc1w = 0, fc1b = fc1w + (int64_t)H * Din, fc2w = fc1b + H, fc2b = fc2w + (int64_t)A * H;
    p.n_params = fc2b + A;
    auto at = [&](int64_t off) { return ws ? ws + off : (float*)nullptr; };
    auto gp = [&](int64_t off) { return dparams ? dparams + off : (float*)nullptr; };
    GJobs& J = p.J;
    J.n = 0;
    J.j[J.n++] = mlg::bjob(at(p.dx), H, inputs, Din, gp(fc1w), gp(fc1b), H, Din, R);
    J.j[J.n++] = mlg::bjob(at(p.gq), A, at(p.x), H, gp(fc2w), gp(fc2b), A, H, R);
    int64_t slab_part;
    const int64_t slab = mlg::layout_bjobs(J, &p.n_tasks, &p.n_red, &slab_part);
    p.nrm = p.slab + slab_part;
    p.total = p.slab + slab;
    return p;
}

template <bool DENSE>
int launch_ff_forward(const MlgAgentDims* d, const float* packed, const float* inputs, const MlgBatch& bt, int t,
                      float* q, int R, hipStream_t s) {
    if (R == 0) return 0;
    const AgentLayout L = make_ff_layout(*d);
    const int tiles = (R + 15) / 16;
    const int grid = (tiles + 3) / 4;
    if (d->hidden == 64)
        hipLaunchKernelGGL((ff_forward_kernel<64, DENSE>), dim3(grid), dim3(256), 0, s, L, packed, inputs, bt, t, q, R);
    else if (d->hidden == 32)
        hipLaunchKernelGGL((ff_forward_kernel<32, DENSE>), dim3(grid), dim3(256), 0, s, L, packed, inputs, bt, t, q, R);
    else
        hipLaunchKernelGGL((ff_forward_kernel<128, DENSE>), dim3(grid), dim3(256), 0, s, L, packed, inputs, bt, t, q, R);
    return mlg::check_launch("ff_forward_kernel");
}

}  // namespace

extern "C" int64_t mlg_ff_packed_size(const MlgAgentDims* d) {
    if (check_agent_dims(d)) return -1;
    return make_ff_layout(*d).total;
}

extern "C" int mlg_ff_pack(const MlgAgentDims* d, const MlgFFParams* p, float* packed, void* stream) {
    if (check_agent_dims(d)) return 1;
    MLG_REQUIRE(p && p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b && packed, "ff_pack: null pointer");
    const AgentLayout L = make_ff_layout(*d);
    hipLaunchKernelGGL(pack_ff_kernel, dim3((unsigned)((L.total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, L, *p,
                       packed);
    return mlg::check_launch("pack_ff_kernel");
}

extern "C" int mlg_ff_forward(const MlgAgentDims* d, const float* packed, const float* inputs, float* q, int32_t R,
                              void* stream) {
    if (check_agent_dims(d)) return 1;
    MLG_REQUIRE(packed && inputs && q && R >= 0, "ff_forward: bad arguments");
    MLG_REQUIRE(mlg::aligned16(packed), "ff_forward: packed must be 16-byte aligned");
    MlgBatch none{};
    return launch_ff_forward<true>(d, packed, inputs, none, 0, q, R, (hipStream_t)stream);
}

extern "C" int mlg_ff_mac_forward(const MlgAgentDims* d, const float* packed, const MlgBatch* batch, int32_t t,
                                  float* q, void* stream) {
    if (check_agent_dims(d)) return 1;
    MLG_REQUIRE(packed && batch && batch->obs && batch->actions_onehot && q, "ff_mac_forward: bad arguments");
    MLG_REQUIRE(mlg::aligned16(packed), "ff_mac_forward: packed must be 16-byte aligned");
    MLG_REQUIRE(batch->B >= 0, "ff_mac_forward: batch B=%d", batch->B);
    MLG_REQUIRE(t >= 0 && t < batch->T1, "ff_mac_forward: t=%d out of [0, %d)", t, batch->T1);
    return launch_ff_forward<false>(d, packed, nullptr, *batch, t, q, batch->B * d->n_agents, (hipStream_t)stream);
}

extern "C" int64_t mlg_ff_backward_workspace_floats(const MlgAgentDims* d, int32_t R) {
    if (check_agent_dims(d)) return -1;
    if (R < 0) {
        mlg::fail("ff_backward: R=%d must be >= 0", R);
        return -1;
    }
    return ff_grad_plan(*d, R, nullptr, nullptr, nullptr).total;
}

extern "C" int mlg_ff_backward(const MlgAgentDims* d, const MlgFFParams* p, const float* packed, const float* inputs,
                               const float* gq, float* d_inputs, float* dparams, float* workspace, int32_t R,
                               void* stream) {
    if (check_agent_dims(d)) return 1;
    MLG_REQUIRE(p && p->fc1_w && p->fc1_b && p->fc2_w && p->fc2_b, "ff_backward: null parameter pointer");
    MLG_REQUIRE(packed && dparams && R >= 0, "ff_backward: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    FFGradPlan pl = ff_grad_plan(*d, R, workspace, inputs, dparams);
    if (R == 0) {
        if (hipMemsetAsync(dparams, 0, (size_t)pl.n_params * sizeof(float), s) != hipSuccess)
            return mlg::fail("ff_backward: zeroing dparams failed");
        return 0;
    }
    MLG_REQUIRE(inputs && workspace, "ff_backward: null inputs / workspace");
    MLG_REQUIRE(mlg::aligned16(workspace) && mlg::aligned16(packed),
                "ff_backward: workspace and packed must be 16-byte aligned");
    const AgentLayout L = make_ff_layout(*d);
    FFGradWs w{workspace + pl.x, workspace + pl.gq, workspace + pl.dx};
    const int tiles = (R + 15) / 16;
    const dim3 grid((unsigned)((tiles + 3) / 4)), block(256);
    if (d->hidden == 64)
        hipLaunchKernelGGL((ff_backward_kernel<64>), grid, block, 0, s, L, packed, inputs, gq, w, d_inputs, R);
    else if (d->hidden == 32)
        hipLaunchKernelGGL((ff_backward_kernel<32>), grid, block, 0, s, L, packed, inputs, gq, w, d_inputs, R);
    else
        hipLaunchKernelGGL((ff_backward_kernel<128>), grid, block, 0, s, L, packed, inputs, gq, w, d_inputs, R);
    if (mlg::check_launch("ff_backward_kernel")) return 1;
    return mlg::run_jobs(pl.J, pl.n_tasks, pl.n_red, workspace + pl.slab, workspace + pl.nrm, s, "ff_backward wgrad");
}
