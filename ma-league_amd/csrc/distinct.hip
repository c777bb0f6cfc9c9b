// distinct.hip -- one agent network per agent slot (mac: distinct, DistinctMAC of
// src/marl/controllers/distinct_agents_controller.py): mlg_mac_forward_distinct and mlg_rollout_distinct.
//
// The weights are a packed pool [N][mlg_packed_agent_size(dims)]: row a is the mlg_pack_agent block of network a
// (mlg_pack_agent_pool writes exactly this). A 16-row MFMA tile shares one weight block, so here a tile is one agent
// across 16 batch rows (MAC forward) or across the 16 envs of a workgroup (rollout, column = env) -- the generic
// kernels' tiles are 16 consecutive (env, agent) rows of the one shared block. The weight view of a tile is
// wave-uniform, selected by the tile's agent. In the rollout a row's arithmetic is agent_device.h's, column by column:
// with N equal networks a run stores the bits of the generic fp32 kernel's.
//
// The rollout has the generic fp32 kernel's structure (rollout.hip's rollout_kernel: a workgroup owns RE = 16 envs for
// the whole episode, env state in LDS, hidden state in VGPRs) with the agent phase agent-major: tile a holds agent a
// of the workgroup's envs, N tiles, wave w owns tiles w, w + 8, .... Weights are read from global memory (N DRQN
// images do not fit in LDS). The selection site is rollout_kernel's own (masked first-index argmax, then
// ro_record_action's epsilon-greedy redraw on the counter RNG, the agent index as the stream index). Env step,
// observation, reset, ring / full-write modes and the run summary are the generic kernel's, bit for bit
// (rollout_env_device.h, rollout_host.h). The body is written out here, not shared with rollout_kernel, for the
// reason rollout_policy.hip records: a shared body changed register allocation in the other instantiations.
//
// No float atomics, no dependence on launch order: two runs from the same state are bit-identical.
#include <cstdlib>
#include <cstring>

#include "agent_device.h"
#include "rollout_env_device.h"
#include "rollout_host.h"

int check_agent_dims(const MlgAgentDims* d);  // agent.hip

namespace {

constexpr int DX_MAX_WAVES = 8, DX_MAX_TPW = 4;

// The MAC forward sums fc1 in the order of DRQNAgentNetwork.forward on the concatenated row (agent_fc1<H, true>: the
// dense block w1d over [obs | onehot], K in steps of 16 from the bias), not in the column-gather order of
// mlg_mac_forward: DistinctMAC's differentiable path calls network i on exactly that row (maleague::drqn_forward), and
// the two paths of one MAC give the same bits. The row is never materialised: element k comes from obs or the one-hot.
__device__ __forceinline__ floatx4 dx_row_chunk(const float* obs, const float* onehot, int k0, int d_obs, int d_in) {
    floatx4 v = {0.f, 0.f, 0.f, 0.f};
    if (!obs) return v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = k0 + r;
        v[r] = k < d_obs ? obs[k] : ((onehot && k < d_in) ? onehot[k - d_obs] : 0.f);
    }
    return v;
}

// agent_cell_hidden<H, true> with the row read through dx_row_chunk: agent_fc1's dense loop, then the ReLU and the
// GRUCell of agent_device.h statement for statement (that header's cell takes its row from one pointer).
template <int H>
__device__ __forceinline__ void dx_cell_dense(const WView& W, const AgentLayout& L, const float* obs,
                                              const float* onehot, floatx4 (&h)[H / 16], int lane) {
    constexpr int HC = H / 16;
    const int col = lane & 15, g = lane >> 4;
    const float* P = W.p;
    floatx4 x[HC];
#pragma unroll
    for (int mt = 0; mt < HC; ++mt) x[mt] = ld4(P + W.b1 + mt * 16 + 4 * g);
    const float* base = P + W.w1d + (int64_t)col * W.ldd + 4 * g;
    for (int kc = 0; kc < L.Dip / 16; ++kc) {
        const floatx4 xin = dx_row_chunk(obs, onehot, kc * 16 + 4 * g, L.d_obs, L.d_in);
#pragma unroll
        for (int mt = 0; mt < HC; ++mt)
            x[mt] = mfma_chunk(ld4(base + (int64_t)mt * 16 * W.ldd + kc * 16), xin, x[mt]);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int mt = 0; mt < HC; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) x[mt][r] = fmaxf(x[mt][r], 0.f);
    floatx4 hn[HC];
    const int64_t gate = (int64_t)H * W.ldh;  // row offset between the r, z and n blocks
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
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float rg = 1.f / (1.f + expf(-ar[r]));
            const float zg = 1.f / (1.f + expf(-az[r]));
            const float ng = tanhf(ain[r] + rg * ahn[r]);
            hn[mt][r] = ng + zg * (h[mt][r] - ng);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int mt = 0; mt < HC; ++mt) h[mt] = hn[mt];
}

// BasicMAC-style forward with network a for agent a: one wave per tile, tile = (agent a, 16 batch rows).
// Inputs built from the batch at t (obs, onehot(a_{t-1})); h [B][N][H].
template <int H>
__global__ void __launch_bounds__(256) mac_forward_distinct_kernel(AgentLayout L, const float* __restrict__ pool,
                                                                  MlgBatch bt, int t, const float* __restrict__ h_in,
                                                                  float* __restrict__ q, float* __restrict__ h_out,
                                                                  int tiles_per_agent, int n_tiles) {
    constexpr int HC = H / 16;
    const int lane = threadIdx.x & 63;
    const int tile = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    if (tile >= n_tiles) return;  // whole wave exits together
    const int N = L.N, B = bt.B;
    const int a = tile / tiles_per_agent, b0 = (tile % tiles_per_agent) * 16;  // wave-uniform
    const int col = lane & 15, g = lane >> 4;
    const int b = b0 + col;
    const bool valid = b < B;
    const int64_t row = (int64_t)b * N + a;  // of q / h
    const int64_t off = valid ? ((bt.rows ? (int64_t)bt.rows[b] : (int64_t)b) * bt.T1 + t) * N + a : 0;
    const float* obs = valid ? bt.obs + off * L.d_obs : nullptr;
    const float* onehot = (valid && t > 0 && L.last_action) ? bt.actions_onehot + (off - N) * L.A : nullptr;
    floatx4 h[HC];
#pragma unroll
    for (int c = 0; c < HC; ++c) {
        floatx4 v = {0.f, 0.f, 0.f, 0.f};
        if (valid && h_in) v = ld4(h_in + row * H + c * 16 + 4 * g);
        h[c] = v;
    }
    const WView W = global_view(pool + (int64_t)a * L.total, L);
    dx_cell_dense<H>(W, L, obs, onehot, h, lane);
    if (valid) {
#pragma unroll
        for (int c = 0; c < HC; ++c) *reinterpret_cast<floatx4*>(h_out + row * H + c * 16 + 4 * g) = h[c];
    }
    for (int at = 0; at < L.Ap / 16; ++at) {
        const floatx4 qt = agent_q_tile<H>(W, h, at, lane);
        if (!valid) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = at * 16 + 4 * g + r;
            if (k < L.A) q[row * L.A + k] = qt[r];
        }
    }
}

template <int H, int TPW>
__global__ void __launch_bounds__(512) rollout_distinct_kernel(MlgEnvSpec spec, MlgEnvState st, AgentLayout L, Sides sd,
                                                              MlgRunInfo info, int test_mode, RolloutLds lay) {
    constexpr int HC = H / 16;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    SpecShared& SS = *reinterpret_cast<SpecShared*>(smem + lay.env.spec);
    const RoEnv R = env_view(smem, lay.env);
    const int U = spec.U, N = spec.n_agents, A = spec.n_actions, S = 6 * U, DO = 8 * U;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), W = nthr >> 6;
    const int e0 = blockIdx.x * RE;
    const int T1 = sd.bt[0].T1;
    const bool any_full_write = sd.bt[0].full_write != 0;
    load_spec_tables(spec, SS);
    const EnvTables T = make_tables(spec, SS);
    const float inv_p = 1.0f / (float)pow2_at_least(spec.grid);
    ro_reset<RoNoStamps>(T, SS, spec, st, R, sd, e0, inv_p);
    __syncthreads();

    floatx4 h[TPW][HC];
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
        for (int c = 0; c < HC; ++c) h[ti][c] = floatx4{0.f, 0.f, 0.f, 0.f};
    RoNoStamps sp;
    sp.init();
    const int e = lane & 15, g = lane >> 4;  // column = env of the workgroup
    const int n_at = L.Ap / 16;
    int last_t = 0;
    for (int t = 0; t < T1; ++t) {
        // ================= agent phase: tile a = agent a of the envs with status 0 (running) or 1 (final action) ====
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti) {
            const int a = wave + ti * W;  // the tile's agent: wave-uniform
            if (a >= N) continue;
            const bool valid = R.status[e] < 2;  // envs past B carry status 2 from the reset
            if (!__any(valid)) continue;  // wave-uniform skip once every env is done
            // Opaque zero offset per tile: stops LICM/CSE from keeping t- and tile-invariant weight loads
            // live across the episode loop in (spilled) registers.
            int zero = 0;
            asm volatile("" : "+s"(zero));
            const WView Wv = global_view(sd.P[0] + (int64_t)a * L.total + zero, L);
            const MlgBatch bt = sd.bt[0];
            const int64_t bt_off = valid ? ((int64_t)R.slot[e] * T1 + t) * N + a : 0;
            RowIn in;
            in.x = valid ? bt.obs + bt_off * DO : nullptr;
            in.onehot = nullptr;
            in.prev_action = (valid && t > 0) ? R.prev[e * N + a] : -1;
            in.agent = 0;
            agent_cell_hidden<H>(Wv, L, in, h[ti], lane);
            const int32_t* av = valid ? bt.avail + bt_off * A : nullptr;
            ArgmaxState as{-INFINITY, 1 << 30};
            for (int at = 0; at < n_at; ++at) {
                const floatx4 q = agent_q_tile<H>(Wv, h[ti], at, lane);
                argmax_accumulate(as, q, av, at, A, lane);
            }
            const int act = argmax_reduce(as);
            if (valid && g == 0) ro_record_action(spec, R, sd, act, av, e, a, e0 + e, t, test_mode);
        }
        __syncthreads();
        ro_env_step(T, SS, spec, R, sd, info, e0, t, inv_p, sp);
        // full-write mode: slot t+1 of envs that are done (t+1 > episode length) gets zeros
        if (any_full_write && t + 1 < T1) zero_slots(sd, R, e0, t + 1, t + 2, A, S, DO);
        if (tid == 0) ro_list_running(R);
        __syncthreads();
        last_t = t;
        if (!R.misc[0]) break;
    }
    // full-write mode: the remaining slots of every env (all of them are done here)
    for (int x = tid; x < RE; x += nthr) R.stepped[x] = 0;
    __syncthreads();
    if (any_full_write && last_t + 2 < T1) zero_slots(sd, R, e0, last_t + 2, T1, A, S, DO);
    ro_finish(st, R, sd, info, e0, sd.bt[0].B, U);
}

int check_distinct_dims(const MlgAgentDims* dims, const char* who) {
    if (check_agent_dims(dims)) return 1;
    MLG_REQUIRE(dims->obs_agent_id == 0,
                "%s: obs_agent_id must be 0 (distinct agent networks take no agent id: network i is agent i)", who);
    return 0;
}

// ---- the dispatch decision (host only) ------------------------------------------------------------------------------
// plan_distinct is the one place that decides which rollout_distinct_kernel<H, TPW> runs; mlg_rollout_distinct launches
// what it returns and mlg_rollout_distinct_describe reports it.
struct DxPlan {
    AgentLayout L;
    int tpw, waves;  // agent tiles per wave, waves per workgroup
    RolloutLds lay;  // the env part only: weights stay in global memory
    char name[24];
};

int plan_distinct(const MlgEnvSpec* spec, const MlgAgentDims* dims, DxPlan* p) {
    MLG_REQUIRE(dims->n_agents == spec->n_agents && dims->n_actions == spec->n_actions && dims->d_obs == 8 * spec->U,
                "rollout_distinct: agent dims do not match env spec (N=%d/%d A=%d/%d d_obs=%d/%d)", dims->n_agents,
                spec->n_agents, dims->n_actions, spec->n_actions, dims->d_obs, 8 * spec->U);
    p->L = make_agent_layout(*dims);
    const int tiles = spec->n_agents;  // one tile per agent
    MLG_REQUIRE(tiles <= DX_MAX_WAVES * DX_MAX_TPW,
                "rollout_distinct: %d agent tiles (one per agent) > %d: at most %d tiles per wave on %d waves", tiles,
                DX_MAX_WAVES * DX_MAX_TPW, DX_MAX_TPW, DX_MAX_WAVES);
    p->waves = tiles < DX_MAX_WAVES ? tiles : DX_MAX_WAVES;
    p->tpw = (tiles + p->waves - 1) / p->waves;
    p->lay = make_rollout_lds(p->L, spec->U, spec->n_agents, false);
    MLG_REQUIRE((int64_t)p->lay.total * 4 <= LDS_LIMIT_BYTES,
                "rollout_distinct: the env state of %d units does not fit in LDS", spec->U);
    snprintf(p->name, sizeof p->name, "dx-global/tpw%d", p->tpw);
    return 0;
}

template <int H, int TPW>
int launch_distinct(const DxPlan& p, int grid, hipStream_t s, const MlgEnvSpec& spec, const MlgEnvState& st,
                    const Sides& sd, const MlgRunInfo& info, int test_mode) {
    const size_t bytes = (size_t)p.lay.total * 4;
    auto kern = rollout_distinct_kernel<H, TPW>;
    if (int rc = allow_lds(kern, bytes, "rollout_distinct")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(p.waves * 64), bytes, s, spec, st, p.L, sd, info, test_mode, p.lay);
    return 0;
}

}  // namespace

extern "C" int mlg_mac_forward_distinct(const MlgAgentDims* d, const float* packed_pool, const MlgBatch* batch,
                                        int32_t t, const float* h_in, float* q, float* h_out, void* stream) {
    if (check_distinct_dims(d, "mac_forward_distinct")) return 1;
    MLG_REQUIRE(packed_pool && batch && batch->obs && batch->actions_onehot && q && h_out,
                "mac_forward_distinct: bad arguments");
    MLG_REQUIRE(mlg::aligned16(packed_pool), "mac_forward_distinct: packed_pool must be 16-byte aligned");
    MLG_REQUIRE(batch->B >= 0, "mac_forward_distinct: batch B=%d", batch->B);
    MLG_REQUIRE(t >= 0 && t < batch->T1, "mac_forward_distinct: t=%d out of [0, %d)", t, batch->T1);
    if (batch->B == 0) return 0;
    const AgentLayout L = make_agent_layout(*d);
    const int tpa = (batch->B + 15) / 16, tiles = tpa * d->n_agents;
    const int grid = (tiles + 3) / 4;
    hipStream_t s = (hipStream_t)stream;
#define MLG_DX_FWD(HH)                                                                                             \
    hipLaunchKernelGGL(mac_forward_distinct_kernel<HH>, dim3(grid), dim3(256), 0, s, L, packed_pool, *batch, (int)t, \
                       h_in, q, h_out, tpa, tiles)
    if (d->hidden == 64) MLG_DX_FWD(64);
    else if (d->hidden == 32) MLG_DX_FWD(32);
    else MLG_DX_FWD(128);
#undef MLG_DX_FWD
    return mlg::check_launch("mac_forward_distinct_kernel");
}

extern "C" int mlg_rollout_distinct_describe(const MlgEnvSpec* spec, const MlgAgentDims* dims, char* name,
                                             int32_t name_cap, int64_t* lds_bytes) {
    if (check_spec(spec) || check_distinct_dims(dims, "rollout_distinct_describe")) return 1;
    MLG_REQUIRE(name && name_cap > 0 && lds_bytes, "rollout_distinct_describe: null output");
    DxPlan plan;
    if (int rc = plan_distinct(spec, dims, &plan)) return rc;
    MLG_REQUIRE((size_t)name_cap > strlen(plan.name), "rollout_distinct_describe: name buffer of %d bytes too small",
                name_cap);
    strcpy(name, plan.name);
    *lds_bytes = (int64_t)plan.lay.total * 4;
    return 0;
}

extern "C" int mlg_rollout_distinct(const MlgEnvSpec* spec, MlgEnvState* st, const MlgAgentDims* dims,
                                    const float* packed_pool, MlgBatch* batch, MlgRunInfo* info, float epsilon,
                                    int32_t test_mode, void* stream) {
    if (check_spec(spec) || check_state(st) || check_distinct_dims(dims, "rollout_distinct")) return 1;
    MLG_REQUIRE(packed_pool && batch && info, "rollout_distinct: null pointer");
    MLG_REQUIRE(mlg::aligned16(packed_pool), "rollout_distinct: packed_pool must be 16-byte aligned");
    if (check_rollout_batch(batch, spec, st, "rollout_distinct")) return 1;
    MLG_REQUIRE(info->ep_len && info->ret && info->won && info->draw, "rollout_distinct: run info has null tensors");
    DxPlan plan;
    if (int rc = plan_distinct(spec, dims, &plan)) return rc;
    hipStream_t s = (hipStream_t)stream;
    Sides sd;
    sd.bt[0] = sd.bt[1] = *batch;
    sd.P[0] = sd.P[1] = packed_pool;
    sd.eps[0] = sd.eps[1] = test_mode ? 0.f : epsilon;
    sd.ns = 1;
    sd.nh = spec->n_agents;
    const int grid = (st->B + RE - 1) / RE;
    int rc = 0;
#define MLG_RO(HH, TT) rc = launch_distinct<HH, TT>(plan, grid, s, *spec, *st, sd, *info, test_mode ? 1 : 0)
#define MLG_RO_H(HH)                       \
    if (plan.tpw == 1) MLG_RO(HH, 1);      \
    else if (plan.tpw == 2) MLG_RO(HH, 2); \
    else if (plan.tpw == 3) MLG_RO(HH, 3); \
    else MLG_RO(HH, 4)
    if (plan.L.H == 64) {
        MLG_RO_H(64);
    } else if (plan.L.H == 32) {
        MLG_RO_H(32);
    } else {
        MLG_RO_H(128);
    }
#undef MLG_RO_H
#undef MLG_RO
    if (rc) return rc;
    return mlg::check_launch("rollout_distinct_kernel");
}
