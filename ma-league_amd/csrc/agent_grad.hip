// agent_grad.hip -- backward of one DRQN cell step (mlg_agent_backward) and of one QMixer call (mlg_qmix_backward)
// for arbitrary rows and arbitrary upstream gradients: the kernels behind the autograd formulas of
// torch.ops.maleague.drqn_forward / qmix_forward. PyTorch chains the steps; nothing is saved between forward and
// backward -- each backward recomputes its step's activations from the step's inputs.
//
// Both run as a row pass that writes per-row deltas and activations to the workspace, then the weight gradients as
// job lists of wgrad_device.h (one wgrad launch, one fixed-order reduce: deterministic, no float atomics).
#include "agent_device.h"
#include "mlg_host.h"
#include "wgrad_device.h"

int check_agent_dims(const MlgAgentDims* d);  // agent.hip

namespace {

using GJobs = mlg::BJobsT<16>;

// ---- agent step --------------------------------------------------------------------------------------------------
// workspace rows (all [R][...], written by the row pass, read by the wgrad jobs)
struct AgentGradWs {
    float *x, *hc, *hp, *gq, *dgi, *dgh, *dx;
};

// One wave per 16-row tile, f32 MFMA in the forward's orientation (A = weights, B = the tile's rows; D layout: lane
// (col, g) register r of chunk c = feature 16c + 4g + r of row col). Forward recomputed chunk by chunk with the gates
// kept (drqn_agent.py:29-35, torch GRUCell), then
//   dh' = gh_out + W2^T gq;  dn = dh' (1 - z)(1 - n^2);  dz = dh' (h - n) z (1 - z);  dr = dn hn r (1 - r)
//   d_gi = [dr, dz, dn], d_gh = [dr, dz, dn r];  dx = (W_ih^T d_gi) [x > 0];  d_inputs = W1^T dx
//   d_h_in = dh' z + W_hh^T d_gh
// The deltas go to the workspace in [row][feature] order; a lane reads back only what it stored itself (the D layout
// of a delta chunk is the B operand of the next product), so the pass needs no barrier.
template <int H>
__global__ void __launch_bounds__(256) agent_backward_kernel(AgentLayout L, const float* __restrict__ P,
                                                            const float* __restrict__ inputs,
                                                            const float* __restrict__ h_in,
                                                            const float* __restrict__ gq,
                                                            const float* __restrict__ gh_out, AgentGradWs w,
                                                            float* __restrict__ d_inputs, float* __restrict__ d_h_in,
                                                            int R) {
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
    floatx4 h[HC], x[HC];
#pragma unroll
    for (int c = 0; c < HC; ++c) h[c] = (valid && h_in) ? ld4(h_in + rh + c * 16 + 4 * g) : zero;
    const WView W = global_view(P, L);
    agent_fc1<H, true>(W, L, in, x, lane);
#pragma unroll
    for (int c = 0; c < HC; ++c) {
#pragma unroll
        for (int r = 0; r < 4; ++r) x[c][r] = fmaxf(x[c][r], 0.f);
        if (valid) {
            st4(w.x + rh + c * 16 + 4 * g, x[c]);
            st4(w.hc + rh + c * 16 + 4 * g, h[c]);
        }
    }
    const float* gqr = (valid && gq) ? gq + (int64_t)row * L.A : nullptr;
    if (valid)
        for (int a = g; a < L.A; a += 4) w.gq[(int64_t)row * L.A + a] = gqr ? gqr[a] : 0.f;
    // ---- gates and gate deltas, one 16-feature chunk at a time ----
    floatx4 dhz[HC];  // dh' z, the direct term of d_h_in
    const int64_t gate = (int64_t)H * W.ldh;
    const int64_t r3 = (int64_t)row * 3 * H;
#pragma unroll
    for (int mt = 0; mt < HC; ++mt) {
        floatx4 ar = ld4(P + W.brz + mt * 16 + 4 * g);
        floatx4 az = ld4(P + W.brz + H + mt * 16 + 4 * g);
        floatx4 ain = ld4(P + W.bih + 2 * H + mt * 16 + 4 * g);
        floatx4 ahn = ld4(P + W.bhh + 2 * H + mt * 16 + 4 * g);
        const float* wr_i = P + W.wih + (int64_t)(mt * 16 + col) * W.ldh + 4 * g;
        const float* wr_h = P + W.whh + (int64_t)(mt * 16 + col) * W.ldh + 4 * g;
#pragma unroll
        for (int kc = 0; kc < HC; ++kc) {
            const int k0 = kc * 16;
            ar = mfma_chunk(ld4(wr_i + k0), x[kc], ar);
            az = mfma_chunk(ld4(wr_i + gate + k0), x[kc], az);
            ain = mfma_chunk(ld4(wr_i + 2 * gate + k0), x[kc], ain);
            ar = mfma_chunk(ld4(wr_h + k0), h[kc], ar);
            az = mfma_chunk(ld4(wr_h + gate + k0), h[kc], az);
            ahn = mfma_chunk(ld4(wr_h + 2 * gate + k0), h[kc], ahn);
        }
        // dh' = gh_out + W2^T gq (fc2 rows past A are zero in the packed block)
        floatx4 dh = (valid && gh_out) ? ld4(gh_out + rh + mt * 16 + 4 * g) : zero;
        if (gq)
            for (int at = 0; at < L.Ap / 16; ++at)
                dh = mfma_chunk(ld_col4(P + W.w2, at * 16 + 4 * g, W.ldh, mt * 16 + col),
                                load_chunk(gqr, at * 16 + 4 * g, L.A), dh);
        floatx4 hp, dr, dz, dn, dnr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float rg = 1.f / (1.f + expf(-ar[r]));
            const float zg = 1.f / (1.f + expf(-az[r]));
            const float ng = tanhf(ain[r] + rg * ahn[r]);
            hp[r] = ng + zg * (h[mt][r] - ng);
            dn[r] = dh[r] * (1.f - zg) * (1.f - ng * ng);
            dz[r] = dh[r] * (h[mt][r] - ng) * zg * (1.f - zg);
            dr[r] = dn[r] * ahn[r] * rg * (1.f - rg);
            dnr[r] = dn[r] * rg;
            dhz[mt][r] = dh[r] * zg;
        }
        if (valid) {
            const int f = mt * 16 + 4 * g;
            st4(w.hp + rh + f, hp);
            st4(w.dgi + r3 + f, dr);
            st4(w.dgi + r3 + H + f, dz);
            st4(w.dgi + r3 + 2 * H + f, dn);
            st4(w.dgh + r3 + f, dr);
            st4(w.dgh + r3 + H + f, dz);
            st4(w.dgh + r3 + 2 * H + f, dnr);
        }
        __builtin_amdgcn_sched_barrier(0);  // as the forward: no hoisting of the next chunk's weight loads
    }
    // ---- dx = (W_ih^T d_gi) [x > 0], d_h_in = dh' z + W_hh^T d_gh ----
    floatx4 dx[HC];
#pragma unroll
    for (int mt = 0; mt < HC; ++mt) {
        floatx4 ax = zero, ah = dhz[mt];
        for (int kc = 0; kc < 3 * HC; ++kc) {  // K = 3H, gate blocks in order
            const floatx4 di = valid ? ld4(w.dgi + r3 + kc * 16 + 4 * g) : zero;
            const floatx4 dg = valid ? ld4(w.dgh + r3 + kc * 16 + 4 * g) : zero;
            ax = mfma_chunk(ld_col4(P + W.wih, kc * 16 + 4 * g, W.ldh, mt * 16 + col), di, ax);
            ah = mfma_chunk(ld_col4(P + W.whh, kc * 16 + 4 * g, W.ldh, mt * 16 + col), dg, ah);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) dx[mt][r] = x[mt][r] > 0.f ? ax[r] : 0.f;
        if (valid) {
            st4(w.dx + rh + mt * 16 + 4 * g, dx[mt]);
            if (d_h_in) st4(d_h_in + rh + mt * 16 + 4 * g, ah);
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

struct AgentGradPlan {
    int64_t x, hc, hp, gq, dgi, dgh, dx, slab, nrm, total, n_params;
    int n_tasks;
    int64_t n_red;
    GJobs J;
};

// workspace offsets and the job table; ws == nullptr: sizes only
AgentGradPlan agent_grad_plan(const MlgAgentDims& d, int R, float* ws, const float* inputs, float* dparams) {
    AgentGradPlan p{};
    const int H = d.hidden, A = d.n_actions, Din = d.d_in;
    int64_t o = 0;
    auto take = [&](int64_t n) {
        const int64_t at = o;
        o += mlg_align4(n);
        return at;
    };
    p.x = take((int64_t)R * H);
    p.hc = take((int64_t)R * H);
    p.hp = take((int64_t)R * H);
    p.gq = take((int64_t)R * A);
    p.dgi = take((int64_t)R * 3 * H);
    p.dgh = take((int64_t)R * 3 * H);
    p.dx = take((int64_t)R * H);
    p.slab = o;
    // dparams in named_parameters() order: fc1.weight, fc1.bias, gru.weight_ih, gru.weight_hh, gru.bias_ih,
    // gru.bias_hh, fc2.weight, fc2.bias
    const int64_t fc1w = 0, fc1b = fc1w + (int64_t)H * Din, wih = fc1b + H, whh = wih + (int64_t)3 * H * H,
                  bih = whh + (int64_t)3 * H * H, bhh = bih + 3 * H, fc2w = bhh + 3 * H, fc2b = fc2w + (int64_t)A * H;
    p.n_params = fc2b + A;
    auto at = [&](int64_t off) { return ws ? ws + off : (float*)nullptr; };
    auto gp = [&](int64_t off) { return dparams ? dparams + off : (float*)nullptr; };
    GJobs& J = p.J;
    J.n = 0;
    J.j[J.n++] = mlg::bjob(at(p.dx), H, inputs, Din, gp(fc1w), gp(fc1b), H, Din, R);
    J.j[J.n++] = mlg::bjob(at(p.dgi), 3 * H, at(p.x), H, gp(wih), gp(bih), 3 * H, H, R);
    J.j[J.n++] = mlg::bjob(at(p.dgh), 3 * H, at(p.hc), H, gp(whh), gp(bhh), 3 * H, H, R);
    J.j[J.n++] = mlg::bjob(at(p.gq), A, at(p.hp), H, gp(fc2w), gp(fc2b), A, H, R);
    int64_t slab_part;
    const int64_t slab = mlg::layout_bjobs(J, &p.n_tasks, &p.n_red, &slab_part);
    p.nrm = p.slab + slab_part;
    p.total = p.slab + slab;
    return p;
}

// ---- QMixer ------------------------------------------------------------------------------------------------------
struct QGradWs {
    float *a1, *af, *hv, *da2, *df2, *dpre, *dv0, *d1a, *d1f;
};

__device__ __forceinline__ float lin_row(const float* w, const float* b, const float* x, int K, int o) {
    float acc = b[o];
    for (int k = 0; k < K; ++k) acc = fmaf(w[(int64_t)o * K + k], x[k], acc);
    return acc;
}
__device__ __forceinline__ float sgn(float v) { return (float)(v > 0.f) - (float)(v < 0.f); }  // sign(0) = 0 (torch)

// One wave per row, lanes over a layer's output features, the row's vectors in LDS: the forward of qmix.py:41-59
// recomputed, then the row's deltas at every linear layer's output and the activations the weight-gradient jobs
// multiply them with, all into the workspace. Every sum runs over its terms in index order, whatever the lane.
//   q_tot = sum_e elu(pre_e) |wf_e| + v,  pre_e = sum_n q_n |w1_ne| + b1_e
//   d pre_e = g |wf_e| elu'(pre_e);  d wf_e = g elu(pre_e) sign(wf_e);  d w1_ne = d pre_e q_n sign(w1_ne)
//   d q_n = sum_e d pre_e |w1_ne|;  hidden ReLU layers of the two-layer hypernets and of V: [pre > 0]
__host__ __device__ inline int qmix_grad_lds_floats(int N, int S, int E, int HE) { return S + 2 * HE + 2 * N * E + 4 * E; }

__global__ void __launch_bounds__(64) qmix_backward_kernel(MlgQMixParams p, const float* __restrict__ qs,
                                                          const float* __restrict__ states,
                                                          const float* __restrict__ g_qtot, QGradWs w,
                                                          float* __restrict__ d_qs, int R) {
    extern __shared__ float lds[];
    const int r = blockIdx.x, lane = threadIdx.x;
    const int N = p.n_agents, S = p.state_dim, E = p.embed_dim, NE = N * E;
    const bool two = p.hypernet_layers == 2;
    const int HE = two ? p.hypernet_embed : 0;
    float* s = lds;        // [S] the row's state
    float* a1 = s + S;     // [HE] relu(hyper_w_1.0 s)
    float* af = a1 + HE;   // [HE] relu(hyper_w_final.0 s)
    float* wp = af + HE;   // [N E] hyper_w_1(s) before abs
    float* da = wp + NE;   // [N E] its delta
    float* dp = da + NE;   // [E] d pre
    float* df = dp + E;    // [E] d wf
    float* b1 = df + E;    // [E] hyper_b_1(s)
    float* wf = b1 + E;    // [E] hyper_w_final(s) before abs
    const float* q = qs + (int64_t)r * N;
    const float g = g_qtot[r];
    for (int k = lane; k < S; k += 64) s[k] = states[(int64_t)r * S + k];
    __syncthreads();
    for (int e = lane; e < E; e += 64) {  // V(s) = v2 . relu(v0 s)
        const float pre = lin_row(p.v0_w, p.v0_b, s, S, e);
        w.hv[(int64_t)r * E + e] = fmaxf(pre, 0.f);
        w.dv0[(int64_t)r * E + e] = pre > 0.f ? g * p.v2_w[e] : 0.f;
        b1[e] = lin_row(p.hb1_w, p.hb1_b, s, S, e);
    }
    for (int k = lane; k < HE; k += 64) {
        a1[k] = fmaxf(lin_row(p.hw1_0w, p.hw1_0b, s, S, k), 0.f);
        af[k] = fmaxf(lin_row(p.hwf_0w, p.hwf_0b, s, S, k), 0.f);
        w.a1[(int64_t)r * HE + k] = a1[k];
        w.af[(int64_t)r * HE + k] = af[k];
    }
    __syncthreads();
    for (int o = lane; o < NE; o += 64)
        wp[o] = two ? lin_row(p.hw1_2w, p.hw1_2b, a1, HE, o) : lin_row(p.hw1_0w, p.hw1_0b, s, S, o);
    for (int e = lane; e < E; e += 64)
        wf[e] = two ? lin_row(p.hwf_2w, p.hwf_2b, af, HE, e) : lin_row(p.hwf_0w, p.hwf_0b, s, S, e);
    __syncthreads();
    for (int e = lane; e < E; e += 64) {
        float acc = 0.f;
        for (int n = 0; n < N; ++n) acc = fmaf(q[n], fabsf(wp[n * E + e]), acc);
        const float pre = acc + b1[e];
        const float hid = pre > 0.f ? pre : expm1f(pre);
        df[e] = g * hid * sgn(wf[e]);
        dp[e] = g * fabsf(wf[e]) * (pre > 0.f ? 1.f : expf(pre));
        w.df2[(int64_t)r * E + e] = df[e];
        w.dpre[(int64_t)r * E + e] = dp[e];
    }
    __syncthreads();
    for (int o = lane; o < NE; o += 64) {
        da[o] = dp[o % E] * q[o / E] * sgn(wp[o]);
        w.da2[(int64_t)r * NE + o] = da[o];
    }
    for (int n = lane; n < N; n += 64) {
        float dq = 0.f;
        for (int e = 0; e < E; ++e) dq = fmaf(dp[e], fabsf(wp[n * E + e]), dq);
        d_qs[(int64_t)r * N + n] = dq;
    }
    if (!two) return;
    __syncthreads();
    for (int k = lane; k < HE; k += 64) {  // back through the second hypernet layers to the hidden ReLUs
        float acc = 0.f;
        for (int o = 0; o < NE; ++o) acc = fmaf(da[o], p.hw1_2w[(int64_t)o * HE + k], acc);
        w.d1a[(int64_t)r * HE + k] = a1[k] > 0.f ? acc : 0.f;
        acc = 0.f;
        for (int e = 0; e < E; ++e) acc = fmaf(df[e], p.hwf_2w[(int64_t)e * HE + k], acc);
        w.d1f[(int64_t)r * HE + k] = af[k] > 0.f ? acc : 0.f;
    }
}

struct QGradPlan {
    int64_t a1, af, hv, da2, df2, dpre, dv0, d1a, d1f, slab, nrm, total, n_params;
    int n_tasks;
    int64_t n_red;
    GJobs J;
};

QGradPlan qmix_grad_plan(const MlgQMixParams& q, int R, float* ws, const float* states, const float* g_qtot,
                         float* dparams) {
    QGradPlan p{};
    const int N = q.n_agents, S = q.state_dim, E = q.embed_dim, HE = q.hypernet_embed;
    const bool two = q.hypernet_layers == 2;
    int64_t o = 0;
    auto take = [&](int64_t n) {
        const int64_t at = o;
        o += mlg_align4(n);
        return at;
    };
    p.a1 = take(two ? (int64_t)R * HE : 0);
    p.af = take(two ? (int64_t)R * HE : 0);
    p.hv = take((int64_t)R * E);
    p.da2 = take((int64_t)R * N * E);
    p.df2 = take((int64_t)R * E);
    p.dpre = take((int64_t)R * E);
    p.dv0 = take((int64_t)R * E);
    p.d1a = take(two ? (int64_t)R * HE : 0);
    p.d1f = take(two ? (int64_t)R * HE : 0);
    p.slab = o;
    auto at = [&](int64_t off) { return ws ? ws + off : (float*)nullptr; };
    int64_t g0 = 0;
    auto gp = [&](int64_t n) {  // the next n floats of dparams
        float* ptr = dparams ? dparams + g0 : nullptr;
        g0 += n;
        return ptr;
    };
    GJobs& J = p.J;
    J.n = 0;
    auto job = [&](const float* delta, int ldd, const float* x, int ldx, int M, int K) {
        float* dw = gp((int64_t)M * K);
        float* db = gp(M);
        J.j[J.n++] = mlg::bjob(delta, ldd, x, ldx, dw, db, M, K, R);
    };
    // dparams in named_parameters() order (two layers: QMIX_ORDER of the learner)
    if (two) {
        job(at(p.d1a), HE, states, S, HE, S);         // hyper_w_1.0
        job(at(p.da2), N * E, at(p.a1), HE, N * E, HE);  // hyper_w_1.2
        job(at(p.d1f), HE, states, S, HE, S);         // hyper_w_final.0
        job(at(p.df2), E, at(p.af), HE, E, HE);       // hyper_w_final.2
    } else {
        job(at(p.da2), N * E, states, S, N * E, S);  // hyper_w_1
        job(at(p.df2), E, states, S, E, S);          // hyper_w_final
    }
    job(at(p.dpre), E, states, S, E, S);  // hyper_b_1
    job(at(p.dv0), E, states, S, E, S);   // V.0
    job(g_qtot, 1, at(p.hv), E, 1, E);    // V.2
    p.n_params = g0;
    int64_t slab_part;
    const int64_t slab = mlg::layout_bjobs(J, &p.n_tasks, &p.n_red, &slab_part);
    p.nrm = p.slab + slab_part;
    p.total = p.slab + slab;
    return p;
}

int check_qmix_dims(const MlgQMixParams* p, const char* what) {
    MLG_REQUIRE(p != nullptr, "%s: null mixer params", what);
    MLG_REQUIRE(p->hypernet_layers == 1 || p->hypernet_layers == 2, "%s: hypernet_layers must be 1 or 2", what);
    MLG_REQUIRE(p->n_agents >= 1 && p->state_dim >= 1 && p->embed_dim >= 1, "%s: invalid mixer dims", what);
    MLG_REQUIRE(p->embed_dim <= 64 && p->hypernet_embed <= 256, "%s: embed dims too large", what);
    MLG_REQUIRE(p->hypernet_layers == 1 || p->hypernet_embed >= 1, "%s: hypernet_embed must be >= 1", what);
    return 0;
}

using mlg::aligned16;
using mlg::run_jobs;

}  // namespace

extern "C" int64_t mlg_agent_backward_workspace_floats(const MlgAgentDims* d, int32_t R) {
    if (check_agent_dims(d)) return -1;
    if (R < 0) {
        mlg::fail("agent_backward: R=%d must be >= 0", R);
        return -1;
    }
    return agent_grad_plan(*d, R, nullptr, nullptr, nullptr).total;
}

extern "C" int mlg_agent_backward(const MlgAgentDims* d, const MlgAgentParams* p, const float* packed,
                                  const float* inputs, const float* h_in, const float* gq, const float* gh_out,
                                  float* d_inputs, float* d_h_in, float* dparams, float* workspace, int32_t R,
                                  void* stream) {
    if (check_agent_dims(d)) return 1;
    MLG_REQUIRE(p && p->fc1_w && p->fc1_b && p->w_ih && p->b_ih && p->w_hh && p->b_hh && p->fc2_w && p->fc2_b,
                "agent_backward: null parameter pointer");
    MLG_REQUIRE(packed && dparams && R >= 0, "agent_backward: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    AgentGradPlan pl = agent_grad_plan(*d, R, workspace, inputs, dparams);
    if (R == 0) {
        if (hipMemsetAsync(dparams, 0, (size_t)pl.n_params * sizeof(float), s) != hipSuccess)
            return mlg::fail("agent_backward: zeroing dparams failed");
        return 0;
    }
    MLG_REQUIRE(inputs && workspace, "agent_backward: null inputs / workspace");
    MLG_REQUIRE(aligned16(workspace) && aligned16(packed) && aligned16(h_in) && aligned16(gh_out) && aligned16(d_h_in),
                "agent_backward: workspace, packed, h_in, gh_out and d_h_in must be 16-byte aligned");
    const AgentLayout L = make_agent_layout(*d);
    AgentGradWs w{workspace + pl.x,   workspace + pl.hc,  workspace + pl.hp, workspace + pl.gq,
                  workspace + pl.dgi, workspace + pl.dgh, workspace + pl.dx};
    const int tiles = (R + 15) / 16;
    const dim3 grid((unsigned)((tiles + 3) / 4)), block(256);
    if (d->hidden == 64)
        hipLaunchKernelGGL((agent_backward_kernel<64>), grid, block, 0, s, L, packed, inputs, h_in, gq, gh_out, w,
                           d_inputs, d_h_in, R);
    else if (d->hidden == 32)
        hipLaunchKernelGGL((agent_backward_kernel<32>), grid, block, 0, s, L, packed, inputs, h_in, gq, gh_out, w,
                           d_inputs, d_h_in, R);
    else
        hipLaunchKernelGGL((agent_backward_kernel<128>), grid, block, 0, s, L, packed, inputs, h_in, gq, gh_out, w,
                           d_inputs, d_h_in, R);
    if (mlg::check_launch("agent_backward_kernel")) return 1;
    return run_jobs(pl.J, pl.n_tasks, pl.n_red, workspace + pl.slab, workspace + pl.nrm, s, "agent_backward wgrad");
}

extern "C" int64_t mlg_qmix_backward_workspace_floats(const MlgQMixParams* p, int32_t R) {
    if (check_qmix_dims(p, "qmix_backward")) return -1;
    if (R < 0) {
        mlg::fail("qmix_backward: R=%d must be >= 0", R);
        return -1;
    }
    return qmix_grad_plan(*p, R, nullptr, nullptr, nullptr, nullptr).total;
}

extern "C" int mlg_qmix_backward(const MlgQMixParams* p, const float* agent_qs, const float* states,
                                 const float* g_qtot, float* d_agent_qs, float* dparams, float* workspace, int32_t R,
                                 void* stream) {
    if (check_qmix_dims(p, "qmix_backward")) return 1;
    MLG_REQUIRE(p->hw1_0w && p->hw1_0b && p->hwf_0w && p->hwf_0b && p->hb1_w && p->hb1_b && p->v0_w && p->v0_b &&
                    p->v2_w && p->v2_b,
                "qmix_backward: null parameter pointer");
    MLG_REQUIRE(p->hypernet_layers == 1 || (p->hw1_2w && p->hw1_2b && p->hwf_2w && p->hwf_2b),
                "qmix_backward: null second-layer parameter pointer");
    MLG_REQUIRE(dparams && R >= 0, "qmix_backward: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    QGradPlan pl = qmix_grad_plan(*p, R, workspace, states, g_qtot, dparams);
    if (R == 0) {
        if (hipMemsetAsync(dparams, 0, (size_t)pl.n_params * sizeof(float), s) != hipSuccess)
            return mlg::fail("qmix_backward: zeroing dparams failed");
        return 0;
    }
    MLG_REQUIRE(agent_qs && states && g_qtot && d_agent_qs && workspace, "qmix_backward: null pointer");
    MLG_REQUIRE(aligned16(workspace), "qmix_backward: workspace must be 16-byte aligned");
    QGradWs w{workspace + pl.a1,   workspace + pl.af,  workspace + pl.hv,  workspace + pl.da2, workspace + pl.df2,
              workspace + pl.dpre, workspace + pl.dv0, workspace + pl.d1a, workspace + pl.d1f};
    const size_t lds = sizeof(float) * (size_t)qmix_grad_lds_floats(p->n_agents, p->state_dim, p->embed_dim,
                                                                   p->hypernet_layers == 2 ? p->hypernet_embed : 0);
    MLG_REQUIRE(lds <= 48 * 1024, "qmix_backward: n_agents * embed_dim + state_dim too large for one row in LDS");
    hipLaunchKernelGGL(qmix_backward_kernel, dim3((unsigned)R), dim3(64), lds, s, *p, agent_qs, states, g_qtot, w,
                       d_agent_qs, R);
    if (mlg::check_launch("qmix_backward_kernel")) return 1;
    return run_jobs(pl.J, pl.n_tasks, pl.n_red, workspace + pl.slab, workspace + pl.nrm, s, "qmix_backward wgrad");
}
