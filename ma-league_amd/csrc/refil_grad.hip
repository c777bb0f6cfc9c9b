// refil_grad.hip -- stand-alone backward of the REFIL layer ops for arbitrary rows and arbitrary upstream gradients:
//
//   mlg_refil_attention_backward  EntityAttentionLayer.forward (src/marl/modules/layers/attention.py:24-79)
//   mlg_refil_agent_backward      one EntityAttentionRNNAgent.forward step (entity_rnn_agent.py:32-65)
//   mlg_refil_mixer_backward      FlexQMixer.forward, plain or with imagine groups (flex_qmix.py:73-117)
//
// the kernels behind the autograd formulas of torch.ops.maleague.refil_attention / entity_agent_forward /
// flex_qmix_forward. As in agent_grad.hip nothing is saved between forward and backward: a row pass (one wave per item
// or per (row, hypernet)) recomputes the forward, writes per-row activations and deltas to the workspace, then every
// weight and bias gradient is a job of wgrad_device.h (one wgrad launch, one fixed-order reduce: deterministic, no
// float atomics).
#include "mlg_host.h"
#include "refil_device.h"
#include "refil_host.h"
#include "wgrad_device.h"

using namespace refil;

namespace {

using GJobs = mlg::BJobsT<16>;

using mlg::aligned16;
using mlg::run_jobs;

// acc[i] (D layout) += sum_k W[k][(mt0 + i) * 16 + 4g + r] * X[col][k] over k < 16 * kchunks: the transposed form of
// mm_lds / mm_reg (W [K][ldw] row-major, the delta rows X in LDS or as D-layout chunks in registers)
template <int MT>
__device__ __forceinline__ void mmT_lds(floatx4 (&acc)[MT], const float* __restrict__ W, int ldw, int mt0, const float* X,
                                        int ldx, int kchunks, int lane) {
    const int col = lane & 15, g = lane >> 4;
    const float* xr = X + col * ldx + 4 * g;
    for (int kc = 0; kc < kchunks; ++kc) {
        const floatx4 xv = ld4(xr + kc * 16);
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[i] = mfma_chunk(ld_col4(W, kc * 16 + 4 * g, ldw, (mt0 + i) * 16 + col), xv, acc[i]);
    }
}

template <int MT, int KC>
__device__ __forceinline__ void mmT_reg(floatx4 (&acc)[MT], const float* __restrict__ W, int ldw, int mt0,
                                        const floatx4 (&x)[KC], int lane) {
    const int col = lane & 15, g = lane >> 4;
#pragma unroll
    for (int kc = 0; kc < KC; ++kc)
#pragma unroll
        for (int i = 0; i < MT; ++i)
            acc[i] = mfma_chunk(ld_col4(W, kc * 16 + 4 * g, ldw, (mt0 + i) * 16 + col), x[kc], acc[i]);
}

// The workspace plan every backward shares: the row pass' buffers first (take, in the op's own order), then the wgrad
// slab of its jobs J (finish). n_params = floats of dparams.
struct GradPlan {
    int64_t slab, nrm, total, n_params;
    int n_tasks;
    int64_t n_red;
    GJobs J;
    int64_t take(int64_t n) {
        const int64_t at = slab;
        slab += mlg_align4(n);
        return at;
    }
    void finish() {
        int64_t slab_part;
        const int64_t n = mlg::layout_bjobs(J, &n_tasks, &n_red, &slab_part);
        nrm = slab + slab_part;
        total = slab + n;
    }
};

// The shape of the three entry points once the dims are checked and the plan is made: an empty batch only zeroes
// dparams; otherwise `rows` checks the remaining pointers and launches the row pass, then the wgrad jobs run.
template <class Rows>
int run_backward(const char* what, const GradPlan& pl, int n, float* dparams, float* ws, hipStream_t s, Rows rows) {
    if (n == 0) {
        if (hipMemsetAsync(dparams, 0, (size_t)pl.n_params * sizeof(float), s) != hipSuccess)
            return mlg::fail("%s: zeroing dparams failed", what);
        return 0;
    }
    MLG_REQUIRE(ws && aligned16(ws), "%s: workspace must be non-null and 16-byte aligned", what);
    if (rows() || mlg::check_launch(what)) return 1;
    return run_jobs(pl.J, pl.n_tasks, pl.n_red, ws + pl.slab, ws + pl.nrm, s, what);
}

// ---- EntityAttentionLayer ------------------------------------------------------------------------------------------
// workspace rows, written by the row pass, read by the wgrad jobs
struct AttnGradWs {
    float *o;     // [bs nq][64]  attention output before out_trans
    float *dout;  // [bs nq][64]  gy with the post-masked rows zeroed
    float *dqkv;  // [bs ne][192] delta at in_trans' output
};

// One wave per item: the forward of attention_kernel (attn_item_fwd, weights P kept in LDS), then dout = gy [row alive];
// dO = W_out^T dout; attn_bwd; dx = W_in^T dqkv. A query row whose every key is masked has P = 0 and passes nothing
// (attention.py:59).
__global__ void __launch_bounds__(64) attention_backward_kernel(const float* __restrict__ w_in,
                                                                const float* __restrict__ w_out,
                                                                const float* __restrict__ x,
                                                                const uint8_t* __restrict__ pre,
                                                                const uint8_t* __restrict__ post, int ne, int nq,
                                                                const float* __restrict__ gy, AttnGradWs w,
                                                                float* __restrict__ dx) {
    __shared__ float s_x[NE * LDX];
    __shared__ float s_qkv[NE * LDQ];
    __shared__ float s_o[16 * LDX];
    __shared__ float s_do[16 * LDX];
    __shared__ float s_dqkv[NE * LDQ];
    __shared__ float s_P[NH * 16 * NE];
    __shared__ float s_ds[NH * 16 * NE];
    __shared__ uint32_t s_m[16];
    const int lane = threadIdx.x;
    const int64_t it = blockIdx.x;
    const int col = lane & 15, g = lane >> 4;
    attn_item_fwd(w_in, x + it * ne * EMB, pre + it * nq * ne, ne, nq, s_x, s_qkv, s_o, s_m, s_P, lane);
    // dout rows (all 16, zeros past nq and for post-masked rows) into s_dqkv as scratch; o and dout rows to the workspace
    const uint32_t dead = mask_row_bits(post + it * nq, nq);
    for (int i = lane; i < 16 * EMB; i += 64) {
        const int q = i / EMB, c = i % EMB;
        const bool live = q < nq && !((dead >> q) & 1u);
        const float d = live ? gy[(it * nq + q) * EMB + c] : 0.f;
        s_dqkv[q * LDQ + c] = d;
        if (q < nq) {
            w.dout[(it * nq + q) * EMB + c] = d;
            w.o[(it * nq + q) * EMB + c] = s_o[q * LDX + c];
        }
    }
    wave_sync();
    floatx4 acc[4];
    zero_acc<4>(acc);
    mmT_lds<4>(acc, w_out, EMB, 0, s_dqkv, LDQ, EMB / 16, lane);  // dO = W_out^T dout
#pragma unroll
    for (int i = 0; i < 4; ++i) st_row(s_do, LDX, i, acc[i], lane);
    wave_sync();
    attn_bwd<false>(s_qkv, s_P, nq, s_do, LDX, s_ds, s_dqkv, lane);
    wave_sync();
    for (int i = lane; i < ne * 3 * EMB; i += 64) {
        const int j = i / (3 * EMB), f = i % (3 * EMB);
        w.dqkv[(it * ne + j) * 3 * EMB + f] = s_dqkv[j * LDQ + f];
    }
    zero_acc<4>(acc);
    mmT_lds<4>(acc, w_in, EMB, 0, s_dqkv, LDQ, 3 * EMB / 16, lane);  // dx = W_in^T dqkv
    if (col < ne) {
#pragma unroll
        for (int i = 0; i < 4; ++i) st4(dx + (it * ne + col) * EMB + i * 16 + 4 * g, acc[i]);
    }
}

struct AttnGradPlan : GradPlan {
    int64_t o, dout, dqkv;
};

AttnGradPlan attn_grad_plan(int bs, int ne, int nq, float* ws, const float* x, float* dparams) {
    AttnGradPlan p{};
    p.o = p.take((int64_t)bs * nq * EMB);
    p.dout = p.take((int64_t)bs * nq * EMB);
    p.dqkv = p.take((int64_t)bs * ne * 3 * EMB);
    // dparams in named_parameters() order: in_trans.weight [192][64], out_trans.weight [64][64], out_trans.bias [64]
    const int64_t win = 0, wout = win + 3 * EMB * EMB, bout = wout + EMB * EMB;
    p.n_params = bout + EMB;
    auto at = [&](int64_t off) { return ws ? ws + off : (float*)nullptr; };
    auto gp = [&](int64_t off) { return dparams ? dparams + off : (float*)nullptr; };
    GJobs& J = p.J;
    J.n = 0;
    J.j[J.n++] = mlg::bjob(at(p.dqkv), 3 * EMB, x, EMB, gp(win), nullptr, 3 * EMB, EMB, bs * ne);
    J.j[J.n++] = mlg::bjob(at(p.dout), EMB, at(p.o), EMB, gp(wout), gp(bout), EMB, EMB, bs * nq);
    p.finish();
    return p;
}

int check_attn_dims(int bs, int ne, int nq, int n_heads, const char* what) {
    MLG_REQUIRE(n_heads == NH, "%s: attn_n_heads=%d unsupported (4; embed 64)", what, n_heads);
    MLG_REQUIRE(ne >= 1 && ne <= NE, "%s: n_entities=%d unsupported (1..16)", what, ne);
    MLG_REQUIRE(nq >= 1 && nq <= 16 && nq <= ne, "%s: nq=%d unsupported (1..min(16, n_entities=%d))", what, nq, ne);
    MLG_REQUIRE(bs >= 0, "%s: bs=%d must be >= 0", what, bs);
    return 0;
}

// ---- EntityAttentionRNNAgent step --------------------------------------------------------------------------------
struct AgentGradWs {
    float *x1;    // [R NE][64]  relu(fc1)
    float *dx1;   // [R NE][64]  delta at fc1's output
    float *dqkv;  // [R NE][192] delta at in_trans' output
    float *o;     // [R NA][64]  attention output
    float *dout;  // [R NA][64]  delta at out_trans' output (zero for masked agents)
    float *x2;    // [R NA][64]  post-masked attention layer output
    float *dx3;   // [R NA][64]  delta at fc2's output
    float *x3;    // [R NA][64]  relu(fc2)
    float *dgi;   // [R NA][192]
    float *dgh;   // [R NA][192]
    float *hp;    // [R NA][64]  h_out
    float *gq;    // [R NA][A]   gq with the masked agents' rows zeroed
};

// One wave per item; the item's NA agent rows are tile rows 0 .. NA - 1 (the rest of the 16-row tile idles). Forward
// recomputed as refil_agent_step_kernel does (f32 MFMA throughout), then, with the GRU formulas of agent_grad.hip,
//   dh' = gh_out + W3^T gq [agent alive];  dn, dz, dr;  d_gi = [dr, dz, dn], d_gh = [dr, dz, dn r]
//   d_h_in = dh' z + W_hh^T d_gh;  dx3 = (W_ih^T d_gi) [x3 > 0];  dout = (W2^T dx3) [agent alive]
//   dO = W_out^T dout;  attn_bwd;  dx1 = (W_in^T dqkv) [x1 > 0]
// An entity-masked agent has q = 0 and a zero attention-layer output (post mask), but its GRU still runs: gh_out of
// such a row reaches h_in, fc2.bias and the GRU weights. The gate deltas go through the workspace; a lane reads
// back only what it stored itself.
__global__ void __launch_bounds__(64) refil_agent_backward_kernel(RAgent L, const float* __restrict__ P, int NA, int NEa,
                                                                  const float* __restrict__ ent,
                                                                  const uint8_t* __restrict__ om,
                                                                  const uint8_t* __restrict__ em,
                                                                  const float* __restrict__ h_in,
                                                                  const float* __restrict__ gq,
                                                                  const float* __restrict__ gh_out, AgentGradWs w,
                                                                  float* __restrict__ d_h_in) {
    __shared__ float s_ein[NE * LDI];
    __shared__ float s_x1[NE * LDX];
    __shared__ float s_qkv[NE * LDQ];
    __shared__ float s_o[16 * LDX];
    __shared__ float s_do[16 * LDX];
    __shared__ float s_dqkv[NE * LDQ];
    __shared__ float s_P[NH * 16 * NE];
    __shared__ float s_ds[NH * 16 * NE];
    __shared__ uint32_t s_m[16];
    const int lane = threadIdx.x;
    const int64_t it = blockIdx.x;
    const int col = lane & 15, g = lane >> 4;
    const int A = L.A;
    const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
    // ---- forward: entity block (attention weights kept) ----
    load_entity_rows(ent + it * NEa * L.D0, NEa, L.D0, L.K1, s_ein, lane, 64);
    zero_tile(s_o, lane);
    if (lane < 16) s_m[lane] = lane < NEa ? mask_row_bits(om + (it * NEa + lane) * NEa, NEa) : 0xFFFFFFFFu;
    wave_sync();
    entity_block(P, L, s_ein, s_x1, s_qkv, s_m, NA, NEa, s_o, s_P, lane);
    for (int i = lane; i < NEa * EMB; i += 64) {
        const int j = i / EMB, c = i % EMB;
        w.x1[(it * NEa + j) * EMB + c] = s_x1[j * LDX + c];
    }
    // ---- forward: agent rows (tile row col = agent col) ----
    const bool valid = col < NA;
    const bool rdead = (dead_rows(mask_row_bits(em + it * NEa, NEa), NA, 16) >> col) & 1u;  // also the rows past NA
    const int64_t row = it * NA + col;
    const int64_t rh = row * EMB, r3 = row * 3 * EMB;
    floatx4 x2[4], x3[4], h[4];
    bias_init<4>(x2, P + L.bout, 0, lane);
    mm_lds<4>(x2, P + L.wout, EMB, 0, s_o, LDX, EMB / 16, lane);
    if (rdead) zero_acc<4>(x2);
    bias_init<4>(x3, P + L.b2, 0, lane);
    mm_reg<4, 4>(x3, P + L.w2, EMB, 0, x2, lane);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        x3[c] = relu4(x3[c]);
        h[c] = valid ? ld4(h_in + rh + c * 16 + 4 * g) : zero;
        if (valid) {
            st4(w.o + rh + c * 16 + 4 * g, ld4(s_o + col * LDX + c * 16 + 4 * g));
            st4(w.x2 + rh + c * 16 + 4 * g, x2[c]);
            st4(w.x3 + rh + c * 16 + 4 * g, x3[c]);
        }
    }
    const float* gqr = (valid && gq && !rdead) ? gq + row * A : nullptr;
    if (valid)
        for (int a = g; a < A; a += 4) w.gq[row * A + a] = gqr ? gqr[a] : 0.f;
    // ---- gates and gate deltas, one 16-feature chunk at a time ----
    floatx4 dhz[4];  // dh' z, the direct term of d_h_in
    const int64_t gate = (int64_t)EMB * EMB;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        floatx4 ar = ld4(P + L.brz + mt * 16 + 4 * g);
        floatx4 az = ld4(P + L.brz + EMB + mt * 16 + 4 * g);
        floatx4 ain = ld4(P + L.bih + 2 * EMB + mt * 16 + 4 * g);
        floatx4 ahn = ld4(P + L.bhh + 2 * EMB + mt * 16 + 4 * g);
        const float* wr_i = P + L.wih + (int64_t)(mt * 16 + col) * EMB + 4 * g;
        const float* wr_h = P + L.whh + (int64_t)(mt * 16 + col) * EMB + 4 * g;
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) {
            const int k0 = kc * 16;
            ar = mfma_chunk(ld4(wr_i + k0), x3[kc], ar);
            az = mfma_chunk(ld4(wr_i + gate + k0), x3[kc], az);
            ain = mfma_chunk(ld4(wr_i + 2 * gate + k0), x3[kc], ain);
            ar = mfma_chunk(ld4(wr_h + k0), h[kc], ar);
            az = mfma_chunk(ld4(wr_h + gate + k0), h[kc], az);
            ahn = mfma_chunk(ld4(wr_h + 2 * gate + k0), h[kc], ahn);
        }
        // dh' = gh_out + W3^T gq (fc3 rows past A are zero in the packed block)
        floatx4 dh = (valid && gh_out) ? ld4(gh_out + rh + mt * 16 + 4 * g) : zero;
        if (gq)
            for (int at = 0; at < L.Ap / 16; ++at)
                dh = mfma_chunk(ld_col4(P + L.w3, at * 16 + 4 * g, EMB, mt * 16 + col),
                                load_chunk(gqr, at * 16 + 4 * g, A), dh);
        floatx4 hp, dr, dz, dn, dnr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float rg = sigm(ar[r]);
            const float zg = sigm(az[r]);
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
            st4(w.dgi + r3 + EMB + f, dz);
            st4(w.dgi + r3 + 2 * EMB + f, dn);
            st4(w.dgh + r3 + f, dr);
            st4(w.dgh + r3 + EMB + f, dz);
            st4(w.dgh + r3 + 2 * EMB + f, dnr);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // ---- dx3 = (W_ih^T d_gi) [x3 > 0], d_h_in = dh' z + W_hh^T d_gh ----
    floatx4 dx3[4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        floatx4 ax = zero, ah = dhz[mt];
        for (int kc = 0; kc < 12; ++kc) {  // K = 3 * 64, gate blocks in order
            const floatx4 di = valid ? ld4(w.dgi + r3 + kc * 16 + 4 * g) : zero;
            const floatx4 dg = valid ? ld4(w.dgh + r3 + kc * 16 + 4 * g) : zero;
            ax = mfma_chunk(ld_col4(P + L.wih, kc * 16 + 4 * g, EMB, mt * 16 + col), di, ax);
            ah = mfma_chunk(ld_col4(P + L.whh, kc * 16 + 4 * g, EMB, mt * 16 + col), dg, ah);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) dx3[mt][r] = x3[mt][r] > 0.f ? ax[r] : 0.f;
        if (valid) {
            st4(w.dx3 + rh + mt * 16 + 4 * g, dx3[mt]);
            if (d_h_in) st4(d_h_in + rh + mt * 16 + 4 * g, ah);
        }
    }
    // ---- dout = (W2^T dx3) [agent alive]; dO = W_out^T dout ----
    floatx4 dout[4], dO[4];
    zero_acc<4>(dout);
    mmT_reg<4, 4>(dout, P + L.w2, EMB, 0, dx3, lane);
    if (rdead) zero_acc<4>(dout);
    zero_acc<4>(dO);
    mmT_reg<4, 4>(dO, P + L.wout, EMB, 0, dout, lane);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        if (valid) st4(w.dout + rh + c * 16 + 4 * g, dout[c]);
        st_row(s_do, LDX, c, dO[c], lane);
    }
    wave_sync();
    attn_bwd<false>(s_qkv, s_P, NA, s_do, LDX, s_ds, s_dqkv, lane);
    wave_sync();
    for (int i = lane; i < NEa * 3 * EMB; i += 64) {
        const int j = i / (3 * EMB), f = i % (3 * EMB);
        w.dqkv[(it * NEa + j) * 3 * EMB + f] = s_dqkv[j * LDQ + f];
    }
    // ---- dx1 = (W_in^T dqkv) [x1 > 0] (tile row col = entity col) ----
    floatx4 acc[4];
    zero_acc<4>(acc);
    mmT_lds<4>(acc, P + L.win, EMB, 0, s_dqkv, LDQ, 3 * EMB / 16, lane);
    if (col < NEa) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const floatx4 xv = ld4(s_x1 + col * LDX + c * 16 + 4 * g);
            floatx4 d;
#pragma unroll
            for (int r = 0; r < 4; ++r) d[r] = xv[r] > 0.f ? acc[c][r] : 0.f;
            st4(w.dx1 + (it * NEa + col) * EMB + c * 16 + 4 * g, d);
        }
    }
}

struct RAgentGradPlan : GradPlan {
    int64_t x1, dx1, dqkv, o, dout, x2, dx3, x3, dgi, dgh, hp, gq;
};

RAgentGradPlan ragent_grad_plan(const MlgRefilDims& d, int R, float* ws, const float* entities, const float* h_in,
                                float* dparams) {
    RAgentGradPlan p{};
    const int NA = d.n_agents, NEa = d.n_entities, A = d.n_actions;
    const RAgent L = make_ragent(refil_d0(&d), A);
    const int64_t re = (int64_t)R * NEa, ra = (int64_t)R * NA;
    p.x1 = p.take(re * EMB);
    p.dx1 = p.take(re * EMB);
    p.dqkv = p.take(re * 3 * EMB);
    p.o = p.take(ra * EMB);
    p.dout = p.take(ra * EMB);
    p.x2 = p.take(ra * EMB);
    p.dx3 = p.take(ra * EMB);
    p.x3 = p.take(ra * EMB);
    p.dgi = p.take(ra * 3 * EMB);
    p.dgh = p.take(ra * 3 * EMB);
    p.hp = p.take(ra * EMB);
    p.gq = p.take(ra * A);
    p.n_params = L.c_total;
    auto at = [&](int64_t off) { return ws ? ws + off : (float*)nullptr; };
    auto gp = [&](int64_t off) { return dparams ? dparams + off : (float*)nullptr; };
    GJobs& J = p.J;
    J.n = 0;
    // dparams in named_parameters() order = the canonical c_* offsets of RAgent
    J.j[J.n++] = mlg::bjob(at(p.dx1), EMB, entities, L.D0, gp(L.c_w1), gp(L.c_b1), EMB, L.D0, (int)re);
    J.j[J.n++] = mlg::bjob(at(p.dqkv), 3 * EMB, at(p.x1), EMB, gp(L.c_win), nullptr, 3 * EMB, EMB, (int)re);
    J.j[J.n++] = mlg::bjob(at(p.dout), EMB, at(p.o), EMB, gp(L.c_wout), gp(L.c_bout), EMB, EMB, (int)ra);
    J.j[J.n++] = mlg::bjob(at(p.dx3), EMB, at(p.x2), EMB, gp(L.c_w2), gp(L.c_b2), EMB, EMB, (int)ra);
    J.j[J.n++] = mlg::bjob(at(p.dgi), 3 * EMB, at(p.x3), EMB, gp(L.c_wih), gp(L.c_bih), 3 * EMB, EMB, (int)ra);
    J.j[J.n++] = mlg::bjob(at(p.dgh), 3 * EMB, h_in, EMB, gp(L.c_whh), gp(L.c_bhh), 3 * EMB, EMB, (int)ra);
    J.j[J.n++] = mlg::bjob(at(p.gq), A, at(p.hp), EMB, gp(L.c_w3), gp(L.c_b3), A, EMB, (int)ra);
    p.finish();
    return p;
}

// ---- FlexQMixer --------------------------------------------------------------------------------------------------
// Three row passes: (A) one wave per (row, hypernet) recomputes the hypernet's output X (hyper_rows_fwd, the forward of
// mixer_fwd_kernel) and writes it to the workspace ([R][5 slots][8 agent rows][32]: w1 (plain or W), w1 I, w_final, b1, V); (B) one 32-lane
// half per row redoes the mixing (flex_qmix.py:91-117) and writes dX per slot and d_agent_qs; (C) one wave per (row,
// hypernet) recomputes the hypernet again with the attention weights kept and walks back through it:
//   dx3 = dX [agent alive];  dout = (W2^T dx3) [agent alive];  dO = W_out^T dout;  attn_bwd;  dx1 = (W_in^T dqkv) [x1 > 0]
// With imagine groups hyper_w_1 runs attention twice (W and I masks, tile rows 0-7 and 8-15) over one qkv; its dqkv is
// the sum of both (attn_bwd<true>) and its agent-row jobs span both copies. (A) and (C) are one kernel template.
struct MixHyperWs {
    float *x1;    // [R NE][64]   relu(fc1)
    float *dx1;   // [R NE][64]
    float *dqkv;  // [R NE][192]
    float *o;     // [R V NA][64] attention output (V = 2 for hyper_w_1 with imagine groups, else 1)
    float *dout;  // [R V NA][64]
    float *x2;    // [R V NA][64] post-masked attention layer output
    float *dx3;   // [R V NA][32] delta at fc2's output
};

struct MixGradArgs {
    int NA, NE, D0, R, softmax, imagine;
    const float* packed;  // 4 RHyper blocks
    const float* qs;      // [R][NA or 2 NA]
    const float* ent;     // [R][NE][D0]
    const uint8_t* em;    // [R][NE]
    const uint8_t* wm;    // [R][NE][NE] or null
    const uint8_t* im;
    const float* g;       // [R]
    float* X;             // [R][5][NAS * EM]
    float* dX;            // [R][5][NAS * EM]
    float* dqs;           // [R][NA or 2 NA]
    MixHyperWs hw[4];
};

template <bool BWD>
__global__ void __launch_bounds__(64) mixer_hyper_kernel(RHyper L, MixGradArgs a) {
    __shared__ float s_ein[NE * LDI];
    __shared__ float s_x1[NE * LDX];
    __shared__ float s_qkv[NE * LDQ];
    __shared__ float s_o[16 * LDX];
    __shared__ float s_P[BWD ? 2 * NH * 16 * NE : 4];
    __shared__ float s_do[BWD ? 16 * LDX : 4];
    __shared__ float s_dqkv[BWD ? NE * LDQ : 4];
    __shared__ float s_ds[BWD ? NH * 16 * NE : 4];
    __shared__ uint32_t s_m[2][16];
    const int lane = threadIdx.x, k = blockIdx.y;
    const int64_t r = blockIdx.x;
    const int col = lane & 15, g = lane >> 4;
    const int NA = a.NA;
    const int V = (k == 0 && a.imagine) ? 2 : 1;
    const floatx4 zero = {0.f, 0.f, 0.f, 0.f};
    const float* P = a.packed + (int64_t)k * L.total;
    const int64_t mrow = r * a.NE * a.NE;
    load_entity_rows(a.ent + r * a.NE * a.D0, a.NE, a.D0, L.K1, s_ein, lane, 64);
    floatx4 x2[4], X[2];
    const uint32_t dead =
        hyper_rows_fwd(P, L, NA, a.NE, a.em + r * a.NE, V == 2 ? a.wm + mrow : nullptr, V == 2 ? a.im + mrow : nullptr,
                       s_ein, s_x1, s_qkv, s_o, s_m, BWD ? s_P : nullptr, lane, x2, X);
    const int v = col >> 3, n = col & 7;
    const int slot = k == 0 ? v : k + 1;
    const int64_t xo = ((r * 5 + slot) * NAS + n) * EM;
    if constexpr (!BWD) {
        if (v < V) {
#pragma unroll
            for (int c = 0; c < 2; ++c) st4(a.X + xo + c * 16 + 4 * g, X[c]);
        }
    } else {
        const MixHyperWs w = a.hw[k];
        const bool valid = v < V && n < NA, active = valid && !((dead >> n) & 1u);  // dead: masked agents, slots past NA
        const int64_t ra = (r * V + v) * NA + n;
        for (int i = lane; i < a.NE * EMB; i += 64) {
            const int j = i / EMB, c = i % EMB;
            w.x1[(r * a.NE + j) * EMB + c] = s_x1[j * LDX + c];
        }
        floatx4 dx3[2], dout[4], dO[4];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            dx3[c] = active ? ld4(a.dX + xo + c * 16 + 4 * g) : zero;
            if (valid) st4(w.dx3 + ra * EM + c * 16 + 4 * g, dx3[c]);
        }
        zero_acc<4>(dout);
        mmT_reg<4, 2>(dout, P + L.w2, EMB, 0, dx3, lane);
        if (!active) zero_acc<4>(dout);
        zero_acc<4>(dO);
        mmT_reg<4, 4>(dO, P + L.wout, EMB, 0, dout, lane);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (valid) {
                st4(w.o + ra * EMB + c * 16 + 4 * g, ld4(s_o + col * LDX + c * 16 + 4 * g));
                st4(w.x2 + ra * EMB + c * 16 + 4 * g, x2[c]);
                st4(w.dout + ra * EMB + c * 16 + 4 * g, dout[c]);
            }
            st_row(s_do, LDX, c, dO[c], lane);
        }
        wave_sync();
        attn_bwd<false>(s_qkv, s_P, NA, s_do, LDX, s_ds, s_dqkv, lane);
        if (V == 2) {
            wave_sync();
            attn_bwd<true>(s_qkv, s_P + NH * 16 * NE, NA, s_do + NAS * LDX, LDX, s_ds, s_dqkv, lane);
        }
        wave_sync();
        for (int i = lane; i < a.NE * 3 * EMB; i += 64) {
            const int j = i / (3 * EMB), f = i % (3 * EMB);
            w.dqkv[(r * a.NE + j) * 3 * EMB + f] = s_dqkv[j * LDQ + f];
        }
        floatx4 acc[4];
        zero_acc<4>(acc);
        mmT_lds<4>(acc, P + L.win, EMB, 0, s_dqkv, LDQ, 3 * EMB / 16, lane);
        if (col < a.NE) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const floatx4 xv = ld4(s_x1 + col * LDX + c * 16 + 4 * g);
                floatx4 d;
#pragma unroll
                for (int q = 0; q < 4; ++q) d[q] = xv[q] > 0.f ? acc[c][q] : 0.f;
                st4(w.dx1 + (r * a.NE + col) * EMB + c * 16 + 4 * g, d);
            }
        }
    }
}

// (B) the mixing (mix_row) and its backward, lane e of a 32-lane half per row (two rows per wave):
//   d v -> g / (NA EM) per element;  d wfp = mw_bwd(g elu(pre));  d pre = g wf elu'(pre);  d b1 rows = d pre / NA
//   d qs_q = sum_e mw(x_q)_e d pre_e;  d x_q = mw_bwd(qs_q d pre)
// The entity-masked agent rows of X are zeros behind a masked_fill: pass (C) drops their dX.
__global__ void __launch_bounds__(64) mixer_mix_backward_kernel(MixGradArgs a) {
    const int e = threadIdx.x & 31;
    const int rr = blockIdx.x * 2 + (threadIdx.x >> 5);
    const bool live = rr < a.R;
    const int r = live ? rr : a.R - 1;  // the spare half of an odd R redoes the last row and stores nothing
    const int NA = a.NA, nrow = a.imagine ? 2 * NA : NA;
    const float* X = a.X + (int64_t)r * 5 * NAS * EM;
    float* dX = a.dX + (int64_t)r * 5 * NAS * EM;
    const float* qs = a.qs + (int64_t)r * nrow;
    const float gr = a.g[r];
    const MixRow m = mix_row(X, qs, NA, nrow, a.softmax, e);
    const float dpre = gr * m.wf * elu_d(m.pre);
    const float dwfp = mw_bwd(gr * m.hid, m.wf, m.wfp, a.softmax);
    const float dv = gr / ((float)NA * (float)EM);
    for (int q = 0; q < NA; ++q) {
        if (live) {
            dX[(2 * NAS + q) * EM + e] = dwfp / (float)NA;
            dX[(3 * NAS + q) * EM + e] = dpre / (float)NA;
            dX[(4 * NAS + q) * EM + e] = dv;
        }
    }
    for (int q = 0; q < nrow; ++q) {
        const int xi = q < NA ? q * EM + e : (NAS + q - NA) * EM + e;
        const float xw = X[xi];
        const float wq = mw(xw, a.softmax);
        const float dq = sum32(wq * dpre);
        const float dxw = mw_bwd(qs[q] * dpre, wq, xw, a.softmax);
        if (live) {
            dX[xi] = dxw;
            if (e == 0) a.dqs[(int64_t)r * nrow + q] = dq;
        }
    }
}

struct MixGradPlan : GradPlan {
    int64_t X, dX;
    int64_t hw[4][7];
};

MixGradPlan mixer_grad_plan(const MlgRefilDims& d, int R, bool imagine, float* ws, const float* entities,
                            float* dparams) {
    MixGradPlan p{};
    const int NA = d.n_agents, NEa = d.n_entities;
    const RHyper L = make_rhyper(refil_d0(&d));
    const int64_t re = (int64_t)R * NEa;
    p.X = p.take((int64_t)R * 5 * NAS * EM);
    p.dX = p.take((int64_t)R * 5 * NAS * EM);
    for (int k = 0; k < 4; ++k) {
        const int64_t ra = (int64_t)R * NA * ((k == 0 && imagine) ? 2 : 1);
        p.hw[k][0] = p.take(re * EMB);
        p.hw[k][1] = p.take(re * EMB);
        p.hw[k][2] = p.take(re * 3 * EMB);
        p.hw[k][3] = p.take(ra * EMB);
        p.hw[k][4] = p.take(ra * EMB);
        p.hw[k][5] = p.take(ra * EMB);
        p.hw[k][6] = p.take(ra * EM);
    }
    p.n_params = 4 * L.c_total;
    auto at = [&](int64_t off) { return ws ? ws + off : (float*)nullptr; };
    GJobs& J = p.J;
    J.n = 0;
    // dparams in named_parameters() order: hyper_w_1, hyper_w_final, hyper_b_1, V, each in the canonical c_* order
    for (int k = 0; k < 4; ++k) {
        const int ra = (int)((int64_t)R * NA * ((k == 0 && imagine) ? 2 : 1));
        auto gp = [&](int64_t off) { return dparams ? dparams + (int64_t)k * L.c_total + off : (float*)nullptr; };
        const int64_t* h = p.hw[k];
        J.j[J.n++] = mlg::bjob(at(h[1]), EMB, entities, L.D0, gp(L.c_w1), gp(L.c_b1), EMB, L.D0, (int)re);
        J.j[J.n++] = mlg::bjob(at(h[2]), 3 * EMB, at(h[0]), EMB, gp(L.c_win), nullptr, 3 * EMB, EMB, (int)re);
        J.j[J.n++] = mlg::bjob(at(h[4]), EMB, at(h[3]), EMB, gp(L.c_wout), gp(L.c_bout), EMB, EMB, ra);
        J.j[J.n++] = mlg::bjob(at(h[6]), EM, at(h[5]), EMB, gp(L.c_w2), gp(L.c_b2), EM, EMB, ra);
    }
    p.finish();
    return p;
}

}  // namespace

extern "C" int64_t mlg_refil_mixer_backward_workspace_floats(const MlgRefilDims* d, int32_t R, int32_t imagine) {
    if (check_refil_mixer_dims(d)) return -1;
    if (R < 0) {
        mlg::fail("refil_mixer_backward: R=%d must be >= 0", R);
        return -1;
    }
    return mixer_grad_plan(*d, R, imagine != 0, nullptr, nullptr, nullptr).total;
}

extern "C" int mlg_refil_mixer_backward(const MlgRefilDims* d, const float* packed, const float* agent_qs,
                                        const float* entities, const uint8_t* entity_mask, const uint8_t* w_mask,
                                        const uint8_t* i_mask, int32_t softmax_mixing_weights, const float* g_qtot,
                                        float* d_agent_qs, float* dparams, float* workspace, int32_t R, void* stream) {
    if (check_refil_mixer_dims(d)) return 1;
    MLG_REQUIRE(packed, "refil_mixer_backward: null packed");
    MLG_REQUIRE(dparams, "refil_mixer_backward: null dparams");
    MLG_REQUIRE(R >= 0, "refil_mixer_backward: R=%d must be >= 0", R);
    MLG_REQUIRE((w_mask == nullptr) == (i_mask == nullptr), "refil_mixer_backward: imagine needs both w_mask and i_mask");
    hipStream_t s = (hipStream_t)stream;
    const bool imagine = w_mask != nullptr;
    const MixGradPlan pl = mixer_grad_plan(*d, R, imagine, workspace, entities, dparams);
    return run_backward("refil_mixer_backward", pl, R, dparams, workspace, s, [&]() -> int {
        MLG_REQUIRE(agent_qs && entities && entity_mask && g_qtot && d_agent_qs,
                    "refil_mixer_backward: null pointer (agent_qs, entities, entity_mask, g_qtot, d_agent_qs)");
        MLG_REQUIRE(aligned16(packed), "refil_mixer_backward: packed must be 16-byte aligned");
        const RHyper L = make_rhyper(refil_d0(d));
        MixGradArgs a{d->n_agents, d->n_entities, L.D0, R, softmax_mixing_weights, imagine, packed, agent_qs, entities,
                      entity_mask, w_mask, i_mask, g_qtot, workspace + pl.X, workspace + pl.dX, d_agent_qs, {}};
        for (int k = 0; k < 4; ++k) {
            const int64_t* h = pl.hw[k];
            a.hw[k] = MixHyperWs{workspace + h[0], workspace + h[1], workspace + h[2], workspace + h[3],
                                 workspace + h[4], workspace + h[5], workspace + h[6]};
        }
        const dim3 grid((unsigned)R, 4);
        hipLaunchKernelGGL(mixer_hyper_kernel<false>, grid, dim3(64), 0, s, L, a);
        hipLaunchKernelGGL(mixer_mix_backward_kernel, dim3((unsigned)((R + 1) / 2)), dim3(64), 0, s, a);
        hipLaunchKernelGGL(mixer_hyper_kernel<true>, grid, dim3(64), 0, s, L, a);
        return 0;
    });
}

extern "C" int64_t mlg_refil_attention_backward_workspace_floats(int32_t bs, int32_t ne, int32_t nq, int32_t n_heads) {
    if (check_attn_dims(bs, ne, nq, n_heads, "refil_attention_backward")) return -1;
    return attn_grad_plan(bs, ne, nq, nullptr, nullptr, nullptr).total;
}

extern "C" int mlg_refil_attention_backward(const float* w_in, const float* w_out, const float* b_out, const float* x,
                                            const uint8_t* pre_mask, const uint8_t* post_mask, const float* gy,
                                            int32_t bs, int32_t ne, int32_t nq, int32_t n_heads, float* dx,
                                            float* dparams, float* workspace, void* stream) {
    if (check_attn_dims(bs, ne, nq, n_heads, "refil_attention_backward")) return 1;
    MLG_REQUIRE(w_in && w_out && b_out, "refil_attention_backward: null parameter pointer (w_in, w_out, b_out)");
    MLG_REQUIRE(dparams, "refil_attention_backward: null dparams");
    hipStream_t s = (hipStream_t)stream;
    const AttnGradPlan pl = attn_grad_plan(bs, ne, nq, workspace, x, dparams);
    return run_backward("refil_attention_backward", pl, bs, dparams, workspace, s, [&]() -> int {
        MLG_REQUIRE(x && pre_mask && post_mask && gy && dx,
                    "refil_attention_backward: null pointer (x, pre_mask, post_mask, gy, dx)");
        MLG_REQUIRE(aligned16(w_in) && aligned16(w_out) && aligned16(dx),
                    "refil_attention_backward: w_in, w_out and dx must be 16-byte aligned");
        AttnGradWs w{workspace + pl.o, workspace + pl.dout, workspace + pl.dqkv};
        hipLaunchKernelGGL(attention_backward_kernel, dim3((unsigned)bs), dim3(64), 0, s, w_in, w_out, x, pre_mask,
                           post_mask, ne, nq, gy, w, dx);
        return 0;
    });
}

extern "C" int64_t mlg_refil_agent_backward_workspace_floats(const MlgRefilDims* d, int32_t R) {
    if (check_refil_dims(d)) return -1;
    if (R < 0) {
        mlg::fail("refil_agent_backward: R=%d must be >= 0", R);
        return -1;
    }
    return ragent_grad_plan(*d, R, nullptr, nullptr, nullptr, nullptr).total;
}

extern "C" int mlg_refil_agent_backward(const MlgRefilDims* d, const float* packed, const float* entities,
                                        const uint8_t* obs_mask, const uint8_t* entity_mask, const float* h_in,
                                        const float* gq, const float* gh_out, float* d_h_in, float* dparams,
                                        float* workspace, int32_t R, void* stream) {
    if (check_refil_dims(d)) return 1;
    MLG_REQUIRE(packed, "refil_agent_backward: null packed");
    MLG_REQUIRE(dparams, "refil_agent_backward: null dparams");
    MLG_REQUIRE(R >= 0, "refil_agent_backward: R=%d must be >= 0", R);
    hipStream_t s = (hipStream_t)stream;
    const RAgentGradPlan pl = ragent_grad_plan(*d, R, workspace, entities, h_in, dparams);
    return run_backward("refil_agent_backward", pl, R, dparams, workspace, s, [&]() -> int {
        MLG_REQUIRE(entities && obs_mask && entity_mask && h_in,
                    "refil_agent_backward: null pointer (entities, obs_mask, entity_mask, h_in)");
        MLG_REQUIRE(aligned16(packed) && aligned16(h_in) && aligned16(gh_out) && aligned16(d_h_in),
                    "refil_agent_backward: packed, h_in, gh_out and d_h_in must be 16-byte aligned");
        AgentGradWs w{workspace + pl.x1,  workspace + pl.dx1, workspace + pl.dqkv, workspace + pl.o,
                      workspace + pl.dout, workspace + pl.x2,  workspace + pl.dx3,  workspace + pl.x3,
                      workspace + pl.dgi, workspace + pl.dgh, workspace + pl.hp,   workspace + pl.gq};
        hipLaunchKernelGGL(refil_agent_backward_kernel, dim3((unsigned)R), dim3(64), 0, s,
                           make_ragent(refil_d0(d), d->n_actions), packed, d->n_agents, d->n_entities, entities, obs_mask,
                           entity_mask, h_in, gq, gh_out, w, d_h_in);
        return 0;
    });
}
