// rollout_policy.hip -- one ParallelStepper.run with a pi_logits MAC (COMA): mlg_rollout_policy, and one
// SelfPlayPolicyParallelStepper.run with two of them: mlg_rollout_selfplay_policy.
//
// The generic fp32 rollout kernel (rollout.hip's rollout_kernel: a workgroup owns RE = 16 envs for the whole episode,
// wave w owns the 16-row agent tiles w, w + W, ..., GRU hidden state in VGPRs, env state in LDS) with the selection
// site replaced: instead of the masked argmax + epsilon-greedy pick, the agent's outputs go through the policy softmax
// with the epsilon floor (MultiAgentController._softmax, multi_agent_controller.py:78-99) and the action is drawn by
// the multinomial rule of mlg_select_multinomial (MultinomialActionSelector.select, action_selectors.py:11-32) on the
// counter RNG, or is the first-index argmax with test_mode and test_greedy. Env step, observation, reset, ring /
// full-write modes and the run summary are the generic kernel's, bit for bit: the env-side device code is
// rollout_env_device.h, the host checks rollout_host.h, both shared with rollout.hip.
#include <cstdlib>
#include <cstring>

#include "agent_device.h"
#include "coma_device.h"
#include "rollout_env_device.h"
#include "rollout_host.h"

int check_agent_dims(const MlgAgentDims* d);  // agent.hip

namespace {

// flags: bit 0 test_mode, bit 1 mask_before_softmax, bit 2 test_greedy. SP = false: one policy side (sd.ns = 1,
// mlg_rollout_policy). SP = true: two policy sides (sd.ns = 2, mlg_rollout_selfplay_policy): side s picks with its own
// weights -- WLDS: the away image follows the home image in LDS -- and its own epsilon floor sd.eps[s]. SP is a
// template flag, not a branch on sd.ns: the SP = false instantiations are the code they were without it.
// The body is rollout_kernel's (rollout.hip) line for line but for the selection site; it is written out twice because
// a shared __forceinline__ body with the selection passed in as a callable made the compiler allocate registers
// differently in every instantiation of both kernels.
template <int H, int TPW, bool WLDS, bool SP = false>
__global__ void __launch_bounds__(512) rollout_policy_kernel(MlgEnvSpec spec, MlgEnvState st, AgentLayout L, Sides sd,
                                                            MlgRunInfo info, int flags, RolloutLds lay) {
    constexpr int HC = H / 16;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    SpecShared& SS = *reinterpret_cast<SpecShared*>(smem + lay.env.spec);
    const RoEnv R = env_view(smem, lay.env);
    const int U = spec.U, N = spec.n_agents, A = spec.n_actions, S = 6 * U, DO = 8 * U, nh = sd.nh;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, W = nthr >> 6;
    const int e0 = blockIdx.x * RE;
    const int T1 = sd.bt[0].T1;
    const bool any_full_write = sd.bt[0].full_write || (sd.ns > 1 && sd.bt[1].full_write);
    load_spec_tables(spec, SS);
    if (WLDS) load_weights_to_lds(sd.P[0], L, lay.lw, reinterpret_cast<float*>(smem + lay.wts));
    if (WLDS && SP) load_weights_to_lds(sd.P[1], L, lay.lw, reinterpret_cast<float*>(smem + lay.wts) + lay.lw.total);
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
    const int tps = (RE * nh + 15) / 16, n_tiles = sd.ns * tps;
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
            const int lds_side = (SP && side) ? lay.lw.total : 0;  // SP: the away image follows the home image
            const WView Wv = WLDS ? lds_view(reinterpret_cast<const float*>(smem + lay.wts) + lds_side + zero, lay.lw, L)
                                  : global_view((side ? sd.P[1] : sd.P[0]) + zero, L);
            const MlgBatch bt = side_batch(sd, side);
            const int64_t bt_off = valid ? ((int64_t)side_slot(R, side, e) * T1 + t) * nh + ln : 0;
            RowIn in;
            in.x = valid ? bt.obs + bt_off * DO : nullptr;
            in.onehot = nullptr;
            in.prev_action = (valid && t > 0) ? R.prev[e * N + a] : -1;
            in.agent = valid ? ln : 0;
            agent_cell_hidden<H>(Wv, L, in, h[ti], lane);
            const int32_t* av = valid ? bt.avail + bt_off * A : nullptr;
            floatx4 qt[RO_MAXAT];
#pragma unroll
            for (int at = 0; at < RO_MAXAT; ++at)
                qt[at] = at < n_at ? agent_q_tile<H>(Wv, h[ti], at, lane) : floatx4{0.f, 0.f, 0.f, 0.f};
            const bool tm = (flags & 1) != 0, greedy = tm && (flags & 4) != 0;
            float u = 0.f;
            if (valid && !greedy)
                u = mlg_u01(mlg_rng(mlg_env_key(spec.seed, e0 + e),
                                    mlg_ctr(R.episode[e], (uint32_t)t, MLG_PURPOSE_POLICY, (uint32_t)a)));
            const float eps = (SP && side) ? sd.eps[1] : sd.eps[0];
            const int act = ro_policy_select(qt, n_at, av, A, lane, eps, (flags & 2) != 0, tm, greedy, u);
            // recorded as a test-mode pick (no epsilon-greedy redraw): the epsilon floor is in the probabilities
            if (valid && g == 0) ro_record_action(spec, R, sd, act, av, e, a, e0 + e, t, 1);
        }
        sp.mark(0);
        __syncthreads();
        sp.mark(1);
        ro_env_step(T, SS, spec, R, sd, info, e0, t, inv_p, sp);
        // full-write mode: slot t+1 of envs that are done (t+1 > episode length) gets zeros
        if (any_full_write && t + 1 < T1) zero_slots(sd, R, e0, t + 1, t + 2, A, S, DO);
        if (tid == 0) ro_list_running(R);
        __syncthreads();
        sp.mark(10);
        last_t = t;
        if (!R.misc[0]) break;
    }
    sp.flush();
    // full-write mode: the remaining slots of every env (all of them are done here)
    for (int e = tid; e < RE; e += nthr) R.stepped[e] = 0;
    __syncthreads();
    if (any_full_write && last_t + 2 < T1) zero_slots(sd, R, e0, last_t + 2, T1, A, S, DO);
    ro_finish(st, R, sd, info, e0, sd.bt[0].B, U);
}


template <int H, int TPW, bool WLDS>
int launch_policy_t(int grid, int threads, hipStream_t s, const MlgEnvSpec& spec, const MlgEnvState& st,
                    const AgentLayout& L, const Sides& sd, const MlgRunInfo& info, int flags, const RolloutLds& lay) {
    const size_t bytes = (size_t)lay.total * 4;
    auto kern = rollout_policy_kernel<H, TPW, WLDS>;
    if (int rc = allow_lds(kern, bytes, "rollout_policy")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), bytes, s, spec, st, L, sd, info, flags, lay);
    return 0;
}

// ---- the dispatch decision (host only) ------------------------------------------------------------------------------
// plan_policy is the one place that decides which rollout_policy_kernel<H, TPW, WLDS> runs; mlg_rollout_policy launches
// what it returns and mlg_rollout_policy_describe reports it.
struct PolicyPlan {
    AgentLayout L;
    int tpw, waves;  // agent tiles per wave, waves per workgroup
    bool wlds;       // the policy's weights in LDS (else read from global memory)
    RolloutLds lay;
    char name[24];
};

// Checks what depends on the spec and the agent dims alone, in the entry point's order. Weights in LDS when the policy's
// image fits next to the env state, else read from HBM / L2.
int plan_policy(const MlgEnvSpec* spec, const MlgAgentDims* dims, PolicyPlan* p) {
    MLG_REQUIRE(dims->n_agents == spec->n_agents && dims->n_actions == spec->n_actions && dims->d_obs == 8 * spec->U,
                "rollout_policy: agent dims do not match env spec (N=%d/%d A=%d/%d d_obs=%d/%d)", dims->n_agents,
                spec->n_agents, dims->n_actions, spec->n_actions, dims->d_obs, 8 * spec->U);
    p->L = make_agent_layout(*dims);
    MLG_REQUIRE(p->L.Ap <= 16 * RO_MAXAT, "rollout_policy: n_actions=%d does not fit %d action tiles", dims->n_actions,
                RO_MAXAT);
    const int tiles = (RE * spec->n_agents + 15) / 16;
    p->waves = tiles < 8 ? tiles : 8;
    p->tpw = (tiles + p->waves - 1) / p->waves;
    MLG_REQUIRE(p->tpw <= 4, "rollout_policy: %d agent tiles per wave > 4 (too many agents per env)", p->tpw);
    MLG_REQUIRE(p->L.H == 32 || p->L.H == 64 || p->L.H == 128,
                "rollout_policy: rnn_hidden_dim=%d unsupported (32, 64, 128)", p->L.H);
    p->lay = make_rollout_lds(p->L, spec->U, spec->n_agents, true);
    p->wlds = p->lay.total * 4 <= LDS_LIMIT_BYTES;
    if (!p->wlds) {
        p->lay = make_rollout_lds(p->L, spec->U, spec->n_agents, false);
        MLG_REQUIRE(p->lay.total * 4 <= LDS_LIMIT_BYTES, "rollout_policy: the env state of %d units does not fit in LDS",
                    spec->U);
    }
    snprintf(p->name, sizeof p->name, "policy-%s/tpw%d", p->wlds ? "lds" : "global", p->tpw);
    return 0;
}

template <int H, int TPW>
int launch_policy(const PolicyPlan& p, int grid, hipStream_t s, const MlgEnvSpec& spec, const MlgEnvState& st,
                  const Sides& sd, const MlgRunInfo& info, int flags) {
    if (p.wlds) return launch_policy_t<H, TPW, true>(grid, p.waves * 64, s, spec, st, p.L, sd, info, flags, p.lay);
    return launch_policy_t<H, TPW, false>(grid, p.waves * 64, s, spec, st, p.L, sd, info, flags, p.lay);
}

// ---- two policy sides: mlg_rollout_selfplay_policy -------------------------------------------------------------------
// plan_selfplay_policy is the one place that decides which rollout_policy_kernel<H, TPW, WLDS, true> runs; the entry
// point launches what it returns and mlg_rollout_selfplay_policy_describe reports it. Checks what depends on the spec
// and the agent dims alone. sp-policy-lds: both sides' images in LDS when they fit next to the env state (H = 32; one
// 3v3 H = 64 image is ~117 KB); sp-policy-global: weights read from HBM / L2, also when MLG_ROLLOUT_GLOBAL_WEIGHTS is
// set (as it forces v1-global in rollout.hip).
// The env is the symmetric two-policy-team scenario and `dims` describes one side of it (rollout.hip's check for
// mlg_rollout_selfplay, under this entry point's name).
int check_selfplay_dims(const MlgEnvSpec* spec, const MlgAgentDims* dims, const char* who) {
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
    return 0;
}

RolloutLds make_selfplay_policy_lds(const AgentLayout& L, int U, int n_agents, bool weights_in_lds) {
    RolloutLds r;
    r.lw = make_lds_weights(L);
    r.weights_in_lds = weights_in_lds;
    int64_t o = 0;
    r.wts = ro_take(o, weights_in_lds ? 2 * (int64_t)r.lw.total : 0);  // home image, then away image
    r.env = make_env_lds(o, U, n_agents);
    r.total = o;
    return r;
}

int plan_selfplay_policy(const MlgEnvSpec* spec, const MlgAgentDims* dims, PolicyPlan* p) {
    if (check_selfplay_dims(spec, dims, "rollout_selfplay_policy")) return 1;
    p->L = make_agent_layout(*dims);
    MLG_REQUIRE(p->L.Ap <= 16 * RO_MAXAT, "rollout_selfplay_policy: n_actions=%d does not fit %d action tiles",
                dims->n_actions, RO_MAXAT);
    const int nh = spec->n_agents / 2;
    const int tiles = 2 * ((RE * nh + 15) / 16);
    p->waves = tiles < 8 ? tiles : 8;
    p->tpw = (tiles + p->waves - 1) / p->waves;
    MLG_REQUIRE(p->tpw <= 4, "rollout_selfplay_policy: %d agent tiles per wave > 4 (more than 16 agents per side)",
                p->tpw);
    MLG_REQUIRE(p->L.H == 32 || p->L.H == 64 || p->L.H == 128,
                "rollout_selfplay_policy: rnn_hidden_dim=%d unsupported (32, 64, 128)", p->L.H);
    p->lay = make_selfplay_policy_lds(p->L, spec->U, spec->n_agents, true);
    // the LDS arm is instantiated for H = 32 alone: two H = 64 images never fit
    p->wlds = p->L.H == 32 && (int64_t)p->lay.total * 4 <= LDS_LIMIT_BYTES && !getenv("MLG_ROLLOUT_GLOBAL_WEIGHTS");
    if (!p->wlds) {
        p->lay = make_selfplay_policy_lds(p->L, spec->U, spec->n_agents, false);
        MLG_REQUIRE((int64_t)p->lay.total * 4 <= LDS_LIMIT_BYTES,
                    "rollout_selfplay_policy: the env state of %d units does not fit in LDS", spec->U);
    }
    snprintf(p->name, sizeof p->name, "sp-policy-%s/tpw%d", p->wlds ? "lds" : "global", p->tpw);
    return 0;
}

template <int H, int TPW>
int launch_selfplay_policy(const PolicyPlan& p, int grid, hipStream_t s, const MlgEnvSpec& spec, const MlgEnvState& st,
                           const Sides& sd, const MlgRunInfo& info, int flags) {
    const size_t bytes = (size_t)p.lay.total * 4;
    auto kern = rollout_policy_kernel<H, TPW, false, true>;
    if constexpr (H == 32) {
        if (p.wlds) kern = rollout_policy_kernel<H, TPW, true, true>;
    }
    if (int rc = allow_lds(kern, bytes, "rollout_selfplay_policy")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(p.waves * 64), bytes, s, spec, st, p.L, sd, info, flags, p.lay);
    return 0;
}

}  // namespace

extern "C" int mlg_rollout_policy_describe(const MlgEnvSpec* spec, const MlgAgentDims* dims, char* name,
                                           int32_t name_cap, int64_t* lds_bytes) {
    if (check_spec(spec) || check_agent_dims(dims)) return 1;
    MLG_REQUIRE(name && name_cap > 0 && lds_bytes, "rollout_policy_describe: null output");
    PolicyPlan plan;
    if (int rc = plan_policy(spec, dims, &plan)) return rc;
    MLG_REQUIRE((size_t)name_cap > strlen(plan.name), "rollout_policy_describe: name buffer of %d bytes too small",
                name_cap);
    strcpy(name, plan.name);
    *lds_bytes = (int64_t)plan.lay.total * 4;
    return 0;
}

extern "C" int mlg_rollout_policy(const MlgEnvSpec* spec, MlgEnvState* st, const MlgAgentDims* dims,
                                  const float* packed, MlgBatch* batch, MlgRunInfo* info, float epsilon,
                                  int32_t test_mode, int32_t mask_before_softmax, int32_t test_greedy, void* stream) {
    if (check_spec(spec) || check_state(st) || check_agent_dims(dims)) return 1;
    MLG_REQUIRE(packed && batch && info, "rollout_policy: null pointer");
    if (check_rollout_batch(batch, spec, st, "rollout_policy")) return 1;
    MLG_REQUIRE(info->ep_len && info->ret && info->won && info->draw, "rollout_policy: run info has null tensors");
    PolicyPlan plan;
    if (int rc = plan_policy(spec, dims, &plan)) return rc;
    hipStream_t s = (hipStream_t)stream;
    Sides sd;
    sd.bt[0] = sd.bt[1] = *batch;
    sd.P[0] = sd.P[1] = packed;
    sd.eps[0] = sd.eps[1] = test_mode ? 0.f : epsilon;
    sd.ns = 1;
    sd.nh = spec->n_agents;
    const int flags = (test_mode ? 1 : 0) | (mask_before_softmax ? 2 : 0) | (test_greedy ? 4 : 0);
    const int grid = (st->B + RE - 1) / RE;
    int rc = 0;
#define MLG_RO(HH, TT) rc = launch_policy<HH, TT>(plan, grid, s, *spec, *st, sd, *info, flags)
#define MLG_RO_H(HH)               \
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
    return mlg::check_launch("rollout_policy_kernel");
}

extern "C" int mlg_rollout_selfplay_policy_describe(const MlgEnvSpec* spec, const MlgAgentDims* dims, char* name,
                                                    int32_t name_cap, int64_t* lds_bytes) {
    if (check_spec(spec) || check_agent_dims(dims)) return 1;
    MLG_REQUIRE(name && name_cap > 0 && lds_bytes, "rollout_selfplay_policy_describe: null output");
    PolicyPlan plan;
    if (int rc = plan_selfplay_policy(spec, dims, &plan)) return rc;
    MLG_REQUIRE((size_t)name_cap > strlen(plan.name),
                "rollout_selfplay_policy_describe: name buffer of %d bytes too small", name_cap);
    strcpy(name, plan.name);
    *lds_bytes = (int64_t)plan.lay.total * 4;
    return 0;
}

extern "C" int mlg_rollout_selfplay_policy(const MlgEnvSpec* spec, MlgEnvState* st, const MlgAgentDims* dims,
                                           const float* home_packed, const float* away_packed, MlgBatch* home,
                                           MlgBatch* away, MlgRunInfo* info, float eps_home, float eps_away,
                                           int32_t test_mode, int32_t mask_before_softmax, int32_t test_greedy,
                                           void* stream) {
    if (check_spec(spec) || check_state(st) || check_agent_dims(dims)) return 1;
    MLG_REQUIRE(home_packed && away_packed && info, "rollout_selfplay_policy: null pointer");
    if (check_rollout_batch(home, spec, st, "rollout_selfplay_policy (home)") ||
        check_rollout_batch(away, spec, st, "rollout_selfplay_policy (away)"))
        return 1;
    MLG_REQUIRE(info->ep_len && info->ret && info->won && info->draw,
                "rollout_selfplay_policy: run info has null tensors");
    PolicyPlan plan;
    if (int rc = plan_selfplay_policy(spec, dims, &plan)) return rc;
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
    const int flags = (test_mode ? 1 : 0) | (mask_before_softmax ? 2 : 0) | (test_greedy ? 4 : 0);
    const int grid = (st->B + RE - 1) / RE;
    int rc = 0;
#define MLG_RO(HH, TT) rc = launch_selfplay_policy<HH, TT>(plan, grid, s, *spec, *st, sd, *info, flags)
#define MLG_RO_H(HH)               \
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
    return mlg::check_launch("rollout_policy_kernel (self-play)");
}
