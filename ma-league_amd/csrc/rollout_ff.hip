// rollout_ff.hip -- one ParallelStepper.run with a feed-forward agent (agent: dqn): mlg_rollout_ff.
//
// The generic fp32 rollout kernel's structure (rollout.hip's rollout_kernel: a workgroup owns RE = 16 envs for the
// whole episode, wave w owns the 16-row agent tiles w, w + W, ..., env state in LDS) with the agent phase replaced:
// agent_fc1, ReLU and agent_q_tile per action tile, and no hidden state carried across steps. The selection site is
// rollout_kernel's own (masked first-index argmax, then ro_record_action's epsilon-greedy redraw on the counter RNG
// with the same purposes and stream indices). Env step, observation, reset, ring / full-write modes and the run
// summary are the generic kernel's, bit for bit: the env-side device code is rollout_env_device.h, the host checks
// rollout_host.h. The body is written out here, not shared with rollout_kernel, for the reason rollout_policy.hip
// records: a shared body changed register allocation in the other instantiations.
//
// The LDS weight image holds w1o, w1a, w1n, b1, w2, b2 only (agent_ff_device.h); without the GRU blocks it is a
// fraction of the DRQN's, so most shapes keep the weights in LDS beside the env state.
#include <cstdlib>
#include <cstring>

#include "agent_ff_device.h"
#include "rollout_env_device.h"
#include "rollout_host.h"

int check_agent_dims(const MlgAgentDims* d);  // agent.hip

namespace {

// Dynamic-LDS layout: the weight image when it fits, then the env part (make_rollout_lds with the feed-forward image).
struct FFRolloutLds {
    int32_t wts, total;
    RoEnvLds env;
    LdsWeights lw;
};

__host__ __device__ inline FFRolloutLds make_ff_rollout_lds(const AgentLayout& L, int U, int n_agents,
                                                            bool weights_in_lds) {
    FFRolloutLds r;
    r.lw = make_ff_lds_weights(L);
    int64_t o = 0;
    r.wts = ro_take(o, weights_in_lds ? r.lw.total : 0);
    r.env = make_env_lds(o, U, n_agents);
    r.total = o;
    return r;
}

template <int H, int TPW, bool WLDS>
__global__ void __launch_bounds__(512) rollout_ff_kernel(MlgEnvSpec spec, MlgEnvState st, AgentLayout L, Sides sd,
                                                        MlgRunInfo info, int test_mode, FFRolloutLds lay) {
    constexpr int HC = H / 16;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    SpecShared& SS = *reinterpret_cast<SpecShared*>(smem + lay.env.spec);
    const RoEnv R = env_view(smem, lay.env);
    const int U = spec.U, N = spec.n_agents, A = spec.n_actions, S = 6 * U, DO = 8 * U, nh = sd.nh;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, W = nthr >> 6;
    const int e0 = blockIdx.x * RE;
    const int T1 = sd.bt[0].T1;
    const bool any_full_write = sd.bt[0].full_write != 0;
    load_spec_tables(spec, SS);
    if (WLDS) load_ff_weights_to_lds(sd.P[0], L, lay.lw, reinterpret_cast<float*>(smem + lay.wts));
    const EnvTables T = make_tables(spec, SS);
    const float inv_p = 1.0f / (float)pow2_at_least(spec.grid);
    ro_reset<RoNoStamps>(T, SS, spec, st, R, sd, e0, inv_p);
    __syncthreads();

    RoNoStamps sp;
    sp.init();
    const int n_tiles = (RE * nh + 15) / 16;  // one policy side
    const int col = lane & 15, g = lane >> 4;
    const int n_at = L.Ap / 16;
    int last_t = 0;
    for (int t = 0; t < T1; ++t) {
        // ================= agent phase: rows of envs with status 0 (running) or 1 (final action) ======
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti) {
            const int tile = wave + ti * W;
            if (tile >= n_tiles) continue;
            const int r = tile * 16 + col;
            const bool in_range = r < RE * nh;
            const int e = in_range ? r / nh : 0, a = r % nh;
            const bool valid = in_range && R.status[e] < 2;
            if (!__any(valid)) continue;  // wave-uniform skip of finished tiles
            // Opaque zero offset per tile: stops LICM/CSE from keeping t- and tile-invariant weight loads
            // live across the episode loop in (spilled) registers.
            int zero = 0;
            asm volatile("" : "+s"(zero));
            const WView Wv = WLDS ? lds_view(reinterpret_cast<const float*>(smem + lay.wts) + zero, lay.lw, L)
                                  : global_view(sd.P[0] + zero, L);
            const MlgBatch bt = sd.bt[0];
            const int64_t bt_off = valid ? ((int64_t)R.slot[e] * T1 + t) * nh + a : 0;
            RowIn in;
            in.x = valid ? bt.obs + bt_off * DO : nullptr;
            in.onehot = nullptr;
            in.prev_action = (valid && t > 0) ? R.prev[e * N + a] : -1;
            in.agent = valid ? a : 0;
            floatx4 x[HC];
            ff_hidden<H, false>(Wv, L, in, x, lane);
            const int32_t* av = valid ? bt.avail + bt_off * A : nullptr;
            ArgmaxState as{-INFINITY, 1 << 30};
            for (int at = 0; at < n_at; ++at) {
                const floatx4 q = agent_q_tile<H>(Wv, x, at, lane);
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
    for (int e = tid; e < RE; e += nthr) R.stepped[e] = 0;
    __syncthreads();
    if (any_full_write && last_t + 2 < T1) zero_slots(sd, R, e0, last_t + 2, T1, A, S, DO);
    ro_finish(st, R, sd, info, e0, sd.bt[0].B, U);
}

template <int H, int TPW, bool WLDS>
int launch_ff_t(int grid, int threads, hipStream_t s, const MlgEnvSpec& spec, const MlgEnvState& st,
                const AgentLayout& L, const Sides& sd, const MlgRunInfo& info, int test_mode, const FFRolloutLds& lay) {
    const size_t bytes = (size_t)lay.total * 4;
    auto kern = rollout_ff_kernel<H, TPW, WLDS>;
    if (int rc = allow_lds(kern, bytes, "rollout_ff")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), bytes, s, spec, st, L, sd, info, test_mode, lay);
    return 0;
}

// ---- the dispatch decision (host only) ------------------------------------------------------------------------------
// plan_ff is the one place that decides which rollout_ff_kernel<H, TPW, WLDS> runs; mlg_rollout_ff launches what it
// returns and mlg_rollout_ff_describe reports it.
struct FFPlan {
    AgentLayout L;
    int tpw, waves;  // agent tiles per wave, waves per workgroup
    bool wlds;       // the weights in LDS (else read from global memory)
    FFRolloutLds lay;
    char name[24];
};

int plan_ff(const MlgEnvSpec* spec, const MlgAgentDims* dims, FFPlan* p) {
    MLG_REQUIRE(dims->n_agents == spec->n_agents && dims->n_actions == spec->n_actions && dims->d_obs == 8 * spec->U,
                "rollout_ff: agent dims do not match env spec (N=%d/%d A=%d/%d d_obs=%d/%d)", dims->n_agents,
                spec->n_agents, dims->n_actions, spec->n_actions, dims->d_obs, 8 * spec->U);
    p->L = make_ff_layout(*dims);
    const int tiles = (RE * spec->n_agents + 15) / 16;
    p->waves = tiles < 8 ? tiles : 8;
    p->tpw = (tiles + p->waves - 1) / p->waves;
    MLG_REQUIRE(p->tpw <= 4, "rollout_ff: %d agent tiles per wave > 4 (too many agents per env)", p->tpw);
    p->lay = make_ff_rollout_lds(p->L, spec->U, spec->n_agents, true);
    p->wlds = (int64_t)p->lay.total * 4 <= LDS_LIMIT_BYTES;
    if (!p->wlds) {
        p->lay = make_ff_rollout_lds(p->L, spec->U, spec->n_agents, false);
        MLG_REQUIRE((int64_t)p->lay.total * 4 <= LDS_LIMIT_BYTES,
                    "rollout_ff: the env state of %d units does not fit in LDS", spec->U);
    }
    snprintf(p->name, sizeof p->name, "ff-%s/tpw%d", p->wlds ? "lds" : "global", p->tpw);
    return 0;
}

template <int H, int TPW>
int launch_ff(const FFPlan& p, int grid, hipStream_t s, const MlgEnvSpec& spec, const MlgEnvState& st, const Sides& sd,
              const MlgRunInfo& info, int test_mode) {
    if (p.wlds) return launch_ff_t<H, TPW, true>(grid, p.waves * 64, s, spec, st, p.L, sd, info, test_mode, p.lay);
    return launch_ff_t<H, TPW, false>(grid, p.waves * 64, s, spec, st, p.L, sd, info, test_mode, p.lay);
}

}  // namespace

extern "C" int mlg_rollout_ff_describe(const MlgEnvSpec* spec, const MlgAgentDims* dims, char* name, int32_t name_cap,
                                       int64_t* lds_bytes) {
    if (check_spec(spec) || check_agent_dims(dims)) return 1;
    MLG_REQUIRE(name && name_cap > 0 && lds_bytes, "rollout_ff_describe: null output");
    FFPlan plan;
    if (int rc = plan_ff(spec, dims, &plan)) return rc;
    MLG_REQUIRE((size_t)name_cap > strlen(plan.name), "rollout_ff_describe: name buffer of %d bytes too small",
                name_cap);
    strcpy(name, plan.name);
    *lds_bytes = (int64_t)plan.lay.total * 4;
    return 0;
}

extern "C" int mlg_rollout_ff(const MlgEnvSpec* spec, MlgEnvState* st, const MlgAgentDims* dims, const float* packed,
                              MlgBatch* batch, MlgRunInfo* info, float epsilon, int32_t test_mode, void* stream) {
    if (check_spec(spec) || check_state(st) || check_agent_dims(dims)) return 1;
    MLG_REQUIRE(packed && batch && info, "rollout_ff: null pointer");
    MLG_REQUIRE(mlg::aligned16(packed), "rollout_ff: packed must be 16-byte aligned");
    if (check_rollout_batch(batch, spec, st, "rollout_ff")) return 1;
    MLG_REQUIRE(info->ep_len && info->ret && info->won && info->draw, "rollout_ff: run info has null tensors");
    FFPlan plan;
    if (int rc = plan_ff(spec, dims, &plan)) return rc;
    hipStream_t s = (hipStream_t)stream;
    Sides sd;
    sd.bt[0] = sd.bt[1] = *batch;
    sd.P[0] = sd.P[1] = packed;
    sd.eps[0] = sd.eps[1] = test_mode ? 0.f : epsilon;
    sd.ns = 1;
    sd.nh = spec->n_agents;
    const int grid = (st->B + RE - 1) / RE;
    int rc = 0;
#define MLG_RO(HH, TT) rc = launch_ff<HH, TT>(plan, grid, s, *spec, *st, sd, *info, test_mode ? 1 : 0)
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
    return mlg::check_launch("rollout_ff_kernel");
}
