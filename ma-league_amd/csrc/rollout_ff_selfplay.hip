// rollout_ff_selfplay.hip -- one SelfPlayParallelStepper.run with two feed-forward MACs (agent: dqn on both sides):
// mlg_rollout_selfplay_ff.
//
// rollout_ff_kernel's structure (rollout_ff.hip: a workgroup owns RE = 16 envs for the whole episode, env state in LDS,
// the agent phase ff_hidden -> agent_q_tile per action tile -> masked first-index argmax -> ro_record_action, no hidden
// state carried) with the two-side tile layout of rollout_policy_kernel's SP = true form (rollout_policy.hip): tps tiles
// per side, tile >= tps is the away side, row r = (tile - side tps) 16 + col is env r / nh, side-local agent r % nh.
// The weight view, the batch and the epsilon of a tile are its side's, wave-uniform; the epsilon RNG stream index is the
// global agent index side nh + ln. Env step, observation, reset, ring / full-write / slot_extent modes, reward[0] /
// reward[1], ret_away and the run summary are rollout_env_device.h's, the host checks rollout_host.h's.
//
// A kernel of its own, not a template flag of rollout_ff_kernel, for the reason rollout_policy.hip records: a shared
// body changed register allocation in the other instantiations.
//
// ffsp-lds: both sides' weight images (agent_ff_device.h: w1o, w1a, w1n, b1, w2, b2) in LDS beside the env state, the
// home image first. ffsp-global: weights read from global memory. The arms differ in where a weight is read from, not
// in the order of any sum.
#include <cstdlib>
#include <cstring>

#include "agent_ff_device.h"
#include "rollout_env_device.h"
#include "rollout_host.h"

int check_agent_dims(const MlgAgentDims* d);  // agent.hip

namespace {

// Dynamic-LDS layout: the two weight images when they fit (home, then away), then the env part.
struct FFSelfplayLds {
    int32_t wts, total;
    RoEnvLds env;
    LdsWeights lw;
};

__host__ __device__ inline FFSelfplayLds make_ff_selfplay_lds(const AgentLayout& L, int U, int n_agents,
                                                              bool weights_in_lds) {
    FFSelfplayLds r;
    r.lw = make_ff_lds_weights(L);
    int64_t o = 0;
    r.wts = ro_take(o, weights_in_lds ? 2 * (int64_t)r.lw.total : 0);
    r.env = make_env_lds(o, U, n_agents);
    r.total = o;
    return r;
}

template <int H, int TPW, bool WLDS>
__global__ void __launch_bounds__(512) rollout_ff_selfplay_kernel(MlgEnvSpec spec, MlgEnvState st, AgentLayout L,
                                                                 Sides sd, MlgRunInfo info, int test_mode,
                                                                 FFSelfplayLds lay) {
    constexpr int HC = H / 16;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    SpecShared& SS = *reinterpret_cast<SpecShared*>(smem + lay.env.spec);
    const RoEnv R = env_view(smem, lay.env);
    const int U = spec.U, N = spec.n_agents, A = spec.n_actions, S = 6 * U, DO = 8 * U, nh = sd.nh;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, W = nthr >> 6;
    const int e0 = blockIdx.x * RE;
    const int T1 = sd.bt[0].T1;
    const bool any_full_write = sd.bt[0].full_write || sd.bt[1].full_write;
    load_spec_tables(spec, SS);
    if (WLDS) {
        float* wl = reinterpret_cast<float*>(smem + lay.wts);
        load_ff_weights_to_lds(sd.P[0], L, lay.lw, wl);
        load_ff_weights_to_lds(sd.P[1], L, lay.lw, wl + lay.lw.total);
    }
    const EnvTables T = make_tables(spec, SS);
    const float inv_p = 1.0f / (float)pow2_at_least(spec.grid);
    ro_reset<RoNoStamps>(T, SS, spec, st, R, sd, e0, inv_p);
    __syncthreads();

    RoNoStamps sp;
    sp.init();
    const int tps = (RE * nh + 15) / 16, n_tiles = 2 * tps;  // tiles per side; tile >= tps: the away side
    const int col = lane & 15, g = lane >> 4;
    const int n_at = L.Ap / 16;
    int last_t = 0;
    for (int t = 0; t < T1; ++t) {
        // ================= agent phase: rows of envs with status 0 (running) or 1 (final action) ======
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti) {
            const int tile = wave + ti * W;
            if (tile >= n_tiles) continue;
            const int side = tile >= tps;
            const int r = (tile - side * tps) * 16 + col;
            const bool in_range = r < RE * nh;
            const int e = in_range ? r / nh : 0, ln = r % nh, a = side * nh + ln;
            const bool valid = in_range && R.status[e] < 2;
            if (!__any(valid)) continue;  // wave-uniform skip of finished tiles
            // Opaque zero offset per tile: stops LICM/CSE from keeping t- and tile-invariant weight loads
            // live across the episode loop in (spilled) registers.
            int zero = 0;
            asm volatile("" : "+s"(zero));
            const int lds_side = side ? lay.lw.total : 0;  // the away image follows the home image
            const WView Wv = WLDS ? lds_view(reinterpret_cast<const float*>(smem + lay.wts) + lds_side + zero, lay.lw, L)
                                  : global_view((side ? sd.P[1] : sd.P[0]) + zero, L);
            const MlgBatch bt = side_batch(sd, side);
            const int64_t bt_off = valid ? ((int64_t)side_slot(R, side, e) * T1 + t) * nh + ln : 0;
            RowIn in;
            in.x = valid ? bt.obs + bt_off * DO : nullptr;
            in.onehot = nullptr;
            in.prev_action = (valid && t > 0) ? R.prev[e * N + a] : -1;
            in.agent = valid ? ln : 0;
            floatx4 x[HC];
            ff_hidden<H, false>(Wv, L, in, x, lane);
            const int32_t* av = valid ? bt.avail + bt_off * A : nullptr;
            ArgmaxState as{-INFINITY, 1 << 30};
            for (int at = 0; at < n_at; ++at) {
                const floatx4 q = agent_q_tile<H>(Wv, x, at, lane);
                argmax_accumulate(as, q, av, at, A, lane);
            }
            const int act = argmax_reduce(as);
            // ro_record_action draws the epsilon-greedy redraw with the side's epsilon on stream index a
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

// ---- the dispatch decision (host only) ------------------------------------------------------------------------------
// plan_ff_selfplay is the one place that decides which rollout_ff_selfplay_kernel<H, TPW, WLDS> runs; the entry point
// launches what it returns and mlg_rollout_selfplay_ff_describe reports it.
struct FFSelfplayPlan {
    AgentLayout L;
    int tpw, waves;  // agent tiles per wave, waves per workgroup
    bool wlds;       // both sides' weights in LDS (else read from global memory)
    FFSelfplayLds lay;
    char name[24];
};

int plan_ff_selfplay(const MlgEnvSpec* spec, const MlgAgentDims* dims, FFSelfplayPlan* p) {
    const char* who = "rollout_selfplay_ff";
    MLG_REQUIRE(spec->n_policy_teams == 2 && spec->n_agents % 2 == 0,
                "%s: %d agents in %d policy teams do not fit the symmetric two-team scenario "
                "(stepper_utils.py:9)", who, spec->n_agents, spec->n_policy_teams);
    const int nh = spec->n_agents / 2;
    MLG_REQUIRE(dims->n_agents == nh && dims->n_actions == spec->n_actions && dims->d_obs == 8 * spec->U,
                "%s: agent dims do not match one side of the env (N=%d/%d A=%d/%d d_obs=%d/%d)", who,
                dims->n_agents, nh, dims->n_actions, spec->n_actions, dims->d_obs, 8 * spec->U);
    for (int a = 0; a < nh; ++a)
        MLG_REQUIRE(spec->team[spec->agent_unit[a]] == spec->policy_team &&
                        spec->team[spec->agent_unit[nh + a]] == 1 - spec->policy_team,
                    "%s: agents 0..%d must be the home team, %d..%d the away team", who, nh - 1, nh, 2 * nh - 1);
    p->L = make_ff_layout(*dims);
    const int tiles = 2 * ((RE * nh + 15) / 16);
    p->waves = tiles < 8 ? tiles : 8;
    p->tpw = (tiles + p->waves - 1) / p->waves;
    MLG_REQUIRE(p->tpw <= 4, "%s: %d agent tiles per wave > 4 (more than 16 agents per side)", who, p->tpw);
    MLG_REQUIRE(p->L.H == 32 || p->L.H == 64 || p->L.H == 128, "%s: rnn_hidden_dim=%d unsupported (32, 64, 128)", who,
                p->L.H);
    p->lay = make_ff_selfplay_lds(p->L, spec->U, spec->n_agents, true);
    p->wlds = (int64_t)p->lay.total * 4 <= LDS_LIMIT_BYTES && !getenv("MLG_ROLLOUT_GLOBAL_WEIGHTS");
    if (!p->wlds) {
        p->lay = make_ff_selfplay_lds(p->L, spec->U, spec->n_agents, false);
        MLG_REQUIRE((int64_t)p->lay.total * 4 <= LDS_LIMIT_BYTES, "%s: the env state of %d units does not fit in LDS",
                    who, spec->U);
    }
    snprintf(p->name, sizeof p->name, "ffsp-%s/tpw%d", p->wlds ? "lds" : "global", p->tpw);
    return 0;
}

template <int H, int TPW>
int launch_ff_selfplay(const FFSelfplayPlan& p, int grid, hipStream_t s, const MlgEnvSpec& spec, const MlgEnvState& st,
                       const Sides& sd, const MlgRunInfo& info, int test_mode) {
    const size_t bytes = (size_t)p.lay.total * 4;
    auto kern = p.wlds ? rollout_ff_selfplay_kernel<H, TPW, true> : rollout_ff_selfplay_kernel<H, TPW, false>;
    if (int rc = allow_lds(kern, bytes, "rollout_selfplay_ff")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(p.waves * 64), bytes, s, spec, st, p.L, sd, info, test_mode, p.lay);
    return 0;
}

}  // namespace

extern "C" int mlg_rollout_selfplay_ff_describe(const MlgEnvSpec* spec, const MlgAgentDims* dims, char* name,
                                                int32_t name_cap, int64_t* lds_bytes) {
    if (check_spec(spec) || check_agent_dims(dims)) return 1;
    MLG_REQUIRE(name && name_cap > 0 && lds_bytes, "rollout_selfplay_ff_describe: null output");
    FFSelfplayPlan plan;
    if (int rc = plan_ff_selfplay(spec, dims, &plan)) return rc;
    MLG_REQUIRE((size_t)name_cap > strlen(plan.name), "rollout_selfplay_ff_describe: name buffer of %d bytes too small",
                name_cap);
    strcpy(name, plan.name);
    *lds_bytes = (int64_t)plan.lay.total * 4;
    return 0;
}

extern "C" int mlg_rollout_selfplay_ff(const MlgEnvSpec* spec, MlgEnvState* st, const MlgAgentDims* dims,
                                       const float* home_packed, const float* away_packed, MlgBatch* home,
                                       MlgBatch* away, MlgRunInfo* info, float eps_home, float eps_away,
                                       int32_t test_mode, void* stream) {
    if (check_spec(spec) || check_state(st) || check_agent_dims(dims)) return 1;
    MLG_REQUIRE(home_packed && away_packed && info, "rollout_selfplay_ff: null pointer");
    MLG_REQUIRE(mlg::aligned16(home_packed) && mlg::aligned16(away_packed),
                "rollout_selfplay_ff: packed weights must be 16-byte aligned");
    if (check_rollout_batch(home, spec, st, "rollout_selfplay_ff (home)") ||
        check_rollout_batch(away, spec, st, "rollout_selfplay_ff (away)"))
        return 1;
    MLG_REQUIRE(info->ep_len && info->ret && info->won && info->draw, "rollout_selfplay_ff: run info has null tensors");
    FFSelfplayPlan plan;
    if (int rc = plan_ff_selfplay(spec, dims, &plan)) return rc;
    hipStream_t s = (hipStream_t)stream;
    Sides sd;
    sd.bt[0] = *home;
    sd.bt[1] = *away;
    sd.P[0] = home_packed;
    sd.P[1] = away_packed;
    sd.eps[0] = test_mode ? 0.f : eps_home;
    sd.eps[1] = test_mode ? 0.f : eps_away;
    sd.ns = 2;
    sd.nh = spec->n_agents / 2;
    const int grid = (st->B + RE - 1) / RE;
    int rc = 0;
#define MLG_RO(HH, TT) rc = launch_ff_selfplay<HH, TT>(plan, grid, s, *spec, *st, sd, *info, test_mode ? 1 : 0)
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
    return mlg::check_launch("rollout_ff_selfplay_kernel");
}
