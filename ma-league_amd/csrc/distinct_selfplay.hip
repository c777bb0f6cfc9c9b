// distinct_selfplay.hip -- one SelfPlayDistinctParallelStepper.run: two DistinctMACs (one DRQN per agent slot on both
// sides) in one launch: mlg_rollout_selfplay_distinct.
//
// mlg_rollout_selfplay on the generic fp32 arm (rollout.hip's rollout_kernel with two sides) with one change: agent ln
// of side s acts with block ln of side s's packed pool [nh][mlg_packed_agent_size(dims)]. The structure is
// rollout_distinct_kernel's (distinct.hip): a workgroup owns RE = 16 envs for the whole episode, env state in LDS,
// hidden state in VGPRs, the agent phase agent-major -- tile a = s nh + ln is agent ln of side s across the workgroup's
// 16 envs (column = env), 2 nh tiles, wave w owns tiles w, w + W, .... A wave's tiles may belong to different sides:
// the side, its batch, its pool and (inside ro_record_action) its epsilon are per tile and wave-uniform. Weights are
// read from global memory through the wave-uniform view sd.P[s] + ln * L.total.
//
// A row's arithmetic is agent_device.h's, column by column (an MFMA column depends on its own row only), the selection
// site is rollout_kernel's own (masked first-index argmax, then ro_record_action's epsilon-greedy redraw on the counter
// RNG with the global agent index s nh + ln as the stream index), and the env phases, ro_record_action, zero_slots and
// ro_finish are rollout_env_device.h's with sd.ns = 2, sd.nh = n_agents / 2: with nh equal networks per side a run
// stores the bits of mlg_rollout_selfplay's generic fp32 kernel. The body is written out here, not shared with
// rollout_kernel or rollout_distinct_kernel, for the reason rollout_policy.hip records: a shared body changed register
// allocation in the other instantiations.
//
// No float atomics, no dependence on launch order: two runs from the same state are bit-identical.
#include <cstdlib>
#include <cstring>

#include "agent_device.h"
#include "rollout_env_device.h"
#include "rollout_host.h"

int check_agent_dims(const MlgAgentDims* d);  // agent.hip

namespace {

constexpr int DXSP_MAX_WAVES = 8, DXSP_MAX_TPW = 4;

template <int H, int TPW>
__global__ void __launch_bounds__(512) rollout_selfplay_distinct_kernel(MlgEnvSpec spec, MlgEnvState st, AgentLayout L,
                                                                       Sides sd, MlgRunInfo info, int test_mode,
                                                                       RolloutLds lay) {
    constexpr int HC = H / 16;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    SpecShared& SS = *reinterpret_cast<SpecShared*>(smem + lay.env.spec);
    const RoEnv R = env_view(smem, lay.env);
    const int U = spec.U, N = spec.n_agents, A = spec.n_actions, S = 6 * U, DO = 8 * U, nh = sd.nh;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), W = nthr >> 6;
    const int e0 = blockIdx.x * RE;
    const int T1 = sd.bt[0].T1;
    const bool any_full_write = sd.bt[0].full_write || sd.bt[1].full_write;
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
        // ===== agent phase: tile a = agent ln of side s in the envs with status 0 (running) or 1 (final action) =====
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti) {
            const int a = wave + ti * W;  // the tile's global agent index s nh + ln: wave-uniform
            if (a >= N) continue;
            const int side = a >= nh, ln = a - side * nh;  // wave-uniform
            const bool valid = R.status[e] < 2;  // envs past B carry status 2 from the reset
            if (!__any(valid)) continue;  // wave-uniform skip once every env is done
            // Opaque zero offset per tile: stops LICM/CSE from keeping t- and tile-invariant weight loads
            // live across the episode loop in (spilled) registers.
            int zero = 0;
            asm volatile("" : "+s"(zero));
            const WView Wv = global_view((side ? sd.P[1] : sd.P[0]) + (int64_t)ln * L.total + zero, L);
            const MlgBatch bt = side_batch(sd, side);
            const int64_t bt_off = valid ? ((int64_t)side_slot(R, side, e) * T1 + t) * nh + ln : 0;
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

int check_dxsp_dims(const MlgAgentDims* dims, const char* who) {
    if (check_agent_dims(dims)) return 1;
    MLG_REQUIRE(dims->obs_agent_id == 0,
                "%s: obs_agent_id must be 0 (distinct agent networks take no agent id: network i is agent i)", who);
    return 0;
}

// ---- the dispatch decision (host only) ------------------------------------------------------------------------------
// plan_dxsp is the one place that decides which rollout_selfplay_distinct_kernel<H, TPW> runs;
// mlg_rollout_selfplay_distinct launches what it returns and mlg_rollout_selfplay_distinct_describe reports it.
struct DxSpPlan {
    AgentLayout L;
    int tpw, waves;  // agent tiles per wave, waves per workgroup
    RolloutLds lay;  // the env part only: weights stay in global memory
    char name[24];
};

// The env is the symmetric two-policy-team scenario and `dims` describes one side of it (rollout.hip's check for
// mlg_rollout_selfplay, under this entry point's name).
int plan_dxsp(const MlgEnvSpec* spec, const MlgAgentDims* dims, DxSpPlan* p) {
    const char* who = "rollout_selfplay_distinct";
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
    p->L = make_agent_layout(*dims);
    MLG_REQUIRE(p->L.H == 32 || p->L.H == 64 || p->L.H == 128, "%s: rnn_hidden_dim=%d unsupported (32, 64, 128)", who,
                p->L.H);
    const int tiles = 2 * nh;  // one tile per agent of either side
    MLG_REQUIRE(tiles <= DXSP_MAX_WAVES * DXSP_MAX_TPW,
                "%s: %d agent tiles (one per agent, %d per side) > %d: at most %d tiles per wave on %d waves", who,
                tiles, nh, DXSP_MAX_WAVES * DXSP_MAX_TPW, DXSP_MAX_TPW, DXSP_MAX_WAVES);
    p->waves = tiles < DXSP_MAX_WAVES ? tiles : DXSP_MAX_WAVES;
    p->tpw = (tiles + p->waves - 1) / p->waves;
    p->lay = make_rollout_lds(p->L, spec->U, spec->n_agents, false);
    MLG_REQUIRE((int64_t)p->lay.total * 4 <= LDS_LIMIT_BYTES, "%s: the env state of %d units does not fit in LDS", who,
                spec->U);
    snprintf(p->name, sizeof p->name, "dxsp-global/tpw%d", p->tpw);
    return 0;
}

template <int H, int TPW>
int launch_dxsp(const DxSpPlan& p, int grid, hipStream_t s, const MlgEnvSpec& spec, const MlgEnvState& st,
                const Sides& sd, const MlgRunInfo& info, int test_mode) {
    const size_t bytes = (size_t)p.lay.total * 4;
    auto kern = rollout_selfplay_distinct_kernel<H, TPW>;
    if (int rc = allow_lds(kern, bytes, "rollout_selfplay_distinct")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(p.waves * 64), bytes, s, spec, st, p.L, sd, info, test_mode, p.lay);
    return 0;
}

}  // namespace

extern "C" int mlg_rollout_selfplay_distinct_describe(const MlgEnvSpec* spec, const MlgAgentDims* dims, char* name,
                                                      int32_t name_cap, int64_t* lds_bytes) {
    if (check_spec(spec) || check_dxsp_dims(dims, "rollout_selfplay_distinct_describe")) return 1;
    MLG_REQUIRE(name && name_cap > 0 && lds_bytes, "rollout_selfplay_distinct_describe: null output");
    DxSpPlan plan;
    if (int rc = plan_dxsp(spec, dims, &plan)) return rc;
    MLG_REQUIRE((size_t)name_cap > strlen(plan.name),
                "rollout_selfplay_distinct_describe: name buffer of %d bytes too small", name_cap);
    strcpy(name, plan.name);
    *lds_bytes = (int64_t)plan.lay.total * 4;
    return 0;
}

extern "C" int mlg_rollout_selfplay_distinct(const MlgEnvSpec* spec, MlgEnvState* st, const MlgAgentDims* dims,
                                             const float* home_pool, const float* away_pool, MlgBatch* home,
                                             MlgBatch* away, MlgRunInfo* info, float eps_home, float eps_away,
                                             int32_t test_mode, void* stream) {
    if (check_spec(spec) || check_state(st) || check_dxsp_dims(dims, "rollout_selfplay_distinct")) return 1;
    MLG_REQUIRE(home_pool && away_pool && info, "rollout_selfplay_distinct: null pointer");
    MLG_REQUIRE(mlg::aligned16(home_pool) && mlg::aligned16(away_pool),
                "rollout_selfplay_distinct: home_pool and away_pool must be 16-byte aligned");
    if (check_rollout_batch(home, spec, st, "rollout_selfplay_distinct (home)") ||
        check_rollout_batch(away, spec, st, "rollout_selfplay_distinct (away)"))
        return 1;
    MLG_REQUIRE(info->ep_len && info->ret && info->won && info->draw,
                "rollout_selfplay_distinct: run info has null tensors");
    DxSpPlan plan;
    if (int rc = plan_dxsp(spec, dims, &plan)) return rc;
    hipStream_t s = (hipStream_t)stream;
    Sides sd;
    sd.bt[0] = *home;
    sd.bt[1] = *away;
    sd.P[0] = home_pool;
    sd.P[1] = away_pool;
    sd.eps[0] = test_mode ? 0.f : eps_home;
    sd.eps[1] = test_mode ? 0.f : eps_away;
    sd.ns = 2;
    sd.nh = spec->n_agents / 2;
    const int grid = (st->B + RE - 1) / RE;
    int rc = 0;
#define MLG_RO(HH, TT) rc = launch_dxsp<HH, TT>(plan, grid, s, *spec, *st, sd, *info, test_mode ? 1 : 0)
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
    return mlg::check_launch("rollout_selfplay_distinct_kernel");
}
