// rollout_mix.hip -- self-play against an opponent mixture: one away policy and one roster per 16 envs.
//
// A league match plays the home policy against one frozen opponent per mlg_rollout_selfplay launch; a player's PFSP
// distribution is then only realised across syncs, every game between two syncs lands in one payoff cell and the home
// replay buffer holds one opponent at a time. mlg_rollout_selfplay_mix plays up to ceil(B / 16) opponents in one
// launch: env b belongs to group b / 16, the group names a row of a packed policy pool (mlg_pack_agent_pool) and a
// spec of a device array (the opponent's roster), as crossplay.hip's pairs do for evaluation. Both EpisodeBatches are
// recorded as in the plain launch.
//
// Two arms, decided on the host in one place (plan_mix):
//   sp8-mix  exactly when mlg_rollout_selfplay would launch sp8 for the shape: rollout_sp8_mix_kernel (rollout.hip,
//            rollout_sp8_mix.inc), one group per sp8 workgroup;
//   v1-mix   everything else: rollout_mix_kernel below, the generic fp32 self-play structure (rollout_kernel<H, TPW,
//            false> of rollout.hip with two sides: 16 envs per workgroup, weights read from global memory), the away
//            weight view and the spec selected per workgroup.
// rollout_mix_kernel's body is written out here and not shared with rollout_kernel for the reason rollout_policy.hip
// and distinct.hip record: a shared body changed the register allocation of the other instantiations. The env phases
// are rollout_env_device.h's; they read the roster through a `const MlgEnvSpec&`, which here is a copy of the group's
// device spec in LDS with the launch's shared scalars written over it. Env b's arithmetic is that of env b of the plain
// launch with (pool[away], specs[spec]) -- same tile layout, same MFMA cell in the same order, same env step, same RNG
// key / counters / stream index -- so its rows and run info are bit-identical to it.
#include <cstdlib>
#include <cstring>

#include "agent_device.h"
#include "rollout_env_device.h"
#include "rollout_host.h"

int check_agent_dims(const MlgAgentDims* d);  // agent.hip
// rollout.hip: sp8's dispatch decision (agents per env of the sp8 instantiation, 0 = not sp8) and the sp8-mix launch
int rollout_selfplay_sp8_shape(const MlgEnvSpec* spec, const MlgAgentDims* dims, int64_t* lds_bytes);
int launch_rollout_sp8_mix(int sn, const MlgEnvSpec* spec0, const MlgEnvState* st, const MlgAgentDims* dims,
                           const float* home_packed, const MlgOpponentMix* mix, const MlgBatch* home,
                           const MlgBatch* away, const MlgRunInfo* info, float eps0, float eps1, int32_t test_mode,
                           void* stream);

namespace {

using Stamps = RoNoStamps;

// What every spec of a launch agrees on (host-checked), as one kernel argument.
struct MixShape {
    int U, N, A, grid, episode_limit, stochastic, policy_team;
    uint64_t seed;
};

struct MixArgs {
    const float* pool;
    int64_t pool_stride;  // floats per packed policy
    const MlgMixGroup* groups;
    const MlgEnvSpec* specs;
    int n_pool, n_specs;
};

constexpr int SPEC_WORDS = (int)(sizeof(MlgEnvSpec) / 4);
static_assert(sizeof(MlgEnvSpec) % 8 == 0, "MlgEnvSpec is copied to LDS as 4-byte words and holds a uint64");

// spec_off: the workgroup's MlgEnvSpec copy, in words after the generic carve (16-byte aligned: ro_take)
template <int H, int TPW>
__global__ void __launch_bounds__(512) rollout_mix_kernel(MixShape sh, MlgEnvState st, AgentLayout L, Sides sd_arg,
                                                         MixArgs mx, MlgRunInfo info, int test_mode, RolloutLds lay,
                                                         int spec_off) {
    constexpr int HC = H / 16;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, W = nthr >> 6;
    const int e0 = blockIdx.x * RE;
    // The host validated its copy of the group table; the launch reads the caller's device copy. A device row that is
    // out of range plays nothing instead of reading past the pool or the spec array.
    const MlgMixGroup grp = mx.groups[blockIdx.x];
    if ((unsigned)grp.away >= (unsigned)mx.n_pool || (unsigned)grp.spec >= (unsigned)mx.n_specs) {
        const int b = e0 + tid;
        if (tid < RE && b < sd_arg.bt[0].B) {
            info.ep_len[b] = -1;
            info.ret[b] = 0.f;
            if (info.ret_away) info.ret_away[b] = 0.f;
            info.won[2 * b] = info.won[2 * b + 1] = 0;
            info.draw[b] = 0;
        }
        return;
    }
    Sides sd = sd_arg;
    sd.P[1] = mx.pool + (int64_t)grp.away * mx.pool_stride;  // wave-uniform
    // the group's spec: its roster tables from device memory, the scalars every spec shares from the kernel argument
    {
        const int* gs = reinterpret_cast<const int*>(mx.specs + grp.spec);
        for (int i = tid; i < SPEC_WORDS; i += nthr) smem[spec_off + i] = gs[i];
        __syncthreads();
        if (tid == 0) {
            MlgEnvSpec& s = *reinterpret_cast<MlgEnvSpec*>(smem + spec_off);
            s.U = sh.U;
            s.n_agents = sh.N;
            s.n_actions = sh.A;
            s.grid = sh.grid;
            s.episode_limit = sh.episode_limit;
            s.stochastic = sh.stochastic;
            s.policy_team = sh.policy_team;
            s.n_policy_teams = 2;
            s.seed = sh.seed;
        }
        __syncthreads();
    }
    const MlgEnvSpec& spec = *reinterpret_cast<const MlgEnvSpec*>(smem + spec_off);
    SpecShared& SS = *reinterpret_cast<SpecShared*>(smem + lay.env.spec);
    const RoEnv R = env_view(smem, lay.env);
    const int U = sh.U, N = sh.N, A = sh.A, S = 6 * U, DO = 8 * U, nh = sd.nh;
    const int T1 = sd.bt[0].T1;
    const bool any_full_write = sd.bt[0].full_write || sd.bt[1].full_write;
    load_spec_tables(spec, SS);
    const EnvTables T = make_tables(spec, SS);
    const float inv_p = 1.0f / (float)pow2_at_least(sh.grid);
    ro_reset<Stamps>(T, SS, spec, st, R, sd, e0, inv_p);
    __syncthreads();

    floatx4 h[TPW][HC];
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
        for (int c = 0; c < HC; ++c) h[ti][c] = floatx4{0.f, 0.f, 0.f, 0.f};
    Stamps sp;
    const int tps = (RE * nh + 15) / 16, n_tiles = 2 * tps;
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
            // opaque zero offset per tile: keeps t- and tile-invariant weight loads out of (spilled) registers
            int zero = 0;
            asm volatile("" : "+s"(zero));
            const WView Wv = global_view((side ? sd.P[1] : sd.P[0]) + zero, L);
            const MlgBatch bt = side_batch(sd, side);
            const int64_t bt_off = valid ? ((int64_t)side_slot(R, side, e) * T1 + t) * nh + ln : 0;
            RowIn in;
            in.x = valid ? bt.obs + bt_off * DO : nullptr;
            in.onehot = nullptr;
            in.prev_action = (valid && t > 0) ? R.prev[e * N + a] : -1;
            in.agent = valid ? ln : 0;
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
    for (int e = tid; e < RE; e += nthr) R.stepped[e] = 0;
    __syncthreads();
    if (any_full_write && last_t + 2 < T1) zero_slots(sd, R, e0, last_t + 2, T1, A, S, DO);
    ro_finish(st, R, sd, info, e0, sd.bt[0].B, U);
}

// ---- the dispatch decision (host only): mlg_rollout_selfplay_mix launches what it returns, the describe call
// reports it ----
struct MixPlan {
    int sn;          // sp8-mix: agents per env of the instantiation (10 / 6); 0: v1-mix
    int tpw, waves;  // v1-mix: agent tiles per wave, waves per workgroup
    RolloutLds lay1;
    int spec_off;
    size_t lds_bytes;
    char name[24];
};

int plan_mix(const MlgEnvSpec* spec0, const MlgAgentDims* dims, MixPlan* p) {
    int64_t lds = 0;
    p->sn = rollout_selfplay_sp8_shape(spec0, dims, &lds);
    if (p->sn) {
        p->lds_bytes = (size_t)lds;
        snprintf(p->name, sizeof p->name, "sp8-mix");
        return 0;
    }
    const AgentLayout L = make_agent_layout(*dims);
    const int nh = spec0->n_agents / 2, tiles = 2 * ((RE * nh + 15) / 16);
    p->waves = tiles < 8 ? tiles : 8;
    p->tpw = (tiles + p->waves - 1) / p->waves;
    MLG_REQUIRE(p->tpw <= 4, "rollout_selfplay_mix: %d agent tiles per wave > 4 (too many agents per env)", p->tpw);
    MLG_REQUIRE(L.H == 32 || L.H == 64 || L.H == 128, "rollout_selfplay_mix: rnn_hidden_dim=%d unsupported (32, 64, 128)",
                L.H);
    p->lay1 = make_rollout_lds(L, spec0->U, spec0->n_agents, false);
    p->spec_off = p->lay1.total;
    p->lds_bytes = ((size_t)p->lay1.total + SPEC_WORDS) * 4;
    MLG_REQUIRE(p->lds_bytes <= (size_t)LDS_LIMIT_BYTES, "rollout_selfplay_mix: U=%d needs %zu B of LDS", spec0->U,
                p->lds_bytes);
    snprintf(p->name, sizeof p->name, "v1-mix/tpw%d", p->tpw);
    return 0;
}

// The symmetric two-team shape mlg_rollout_selfplay asks of its spec, with the home team first.
int check_mix_spec(const MlgEnvSpec* s, const char* what, int k) {
    if (check_spec(s)) return 1;
    MLG_REQUIRE(s->n_policy_teams == 2 && s->n_agents % 2 == 0,
                "rollout_selfplay_mix: %s[%d]: %d agents in %d policy teams do not fit the symmetric two-team scenario",
                what, k, s->n_agents, s->n_policy_teams);
    const int nh = s->n_agents / 2;
    for (int a = 0; a < nh; ++a)
        MLG_REQUIRE(s->team[s->agent_unit[a]] == s->policy_team && s->team[s->agent_unit[nh + a]] == 1 - s->policy_team,
                    "rollout_selfplay_mix: %s[%d]: agents 0..%d must be the home team, %d..%d the away team", what, k,
                    nh - 1, nh, 2 * nh - 1);
    return 0;
}

int check_mix_dims(const MlgEnvSpec* spec0, const MlgAgentDims* dims) {
    if (check_mix_spec(spec0, "spec0", 0) || check_agent_dims(dims)) return 1;
    const int nh = spec0->n_agents / 2;
    MLG_REQUIRE(dims->n_agents == nh && dims->n_actions == spec0->n_actions && dims->d_obs == 8 * spec0->U,
                "rollout_selfplay_mix: agent dims do not match one side of the env (N=%d/%d A=%d/%d d_obs=%d/%d)",
                dims->n_agents, nh, dims->n_actions, spec0->n_actions, dims->d_obs, 8 * spec0->U);
    return 0;
}

template <int H, int TPW>
int launch_mix(int grid, hipStream_t s, const MixShape& sh, const MlgEnvState& st, const AgentLayout& L, const Sides& sd,
               const MixArgs& mx, const MlgRunInfo& info, int tm, const MixPlan& p) {
    auto kern = rollout_mix_kernel<H, TPW>;
    if (int rc = allow_lds(kern, p.lds_bytes, "rollout_selfplay_mix")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(p.waves * 64), p.lds_bytes, s, sh, st, L, sd, mx, info, tm, p.lay1,
                       p.spec_off);
    return 0;
}

}  // namespace

extern "C" int mlg_rollout_selfplay_mix_describe(const MlgEnvSpec* spec0, const MlgAgentDims* dims, char* name,
                                                 int32_t name_cap, int64_t* lds_bytes) {
    MLG_REQUIRE(spec0 && dims, "rollout_selfplay_mix_describe: null spec or dims");
    MLG_REQUIRE(name && name_cap > 0 && lds_bytes, "rollout_selfplay_mix_describe: null output");
    if (check_mix_dims(spec0, dims)) return 1;
    MixPlan plan;
    if (int rc = plan_mix(spec0, dims, &plan)) return rc;
    MLG_REQUIRE((size_t)name_cap > strlen(plan.name), "rollout_selfplay_mix_describe: name buffer of %d bytes too small",
                name_cap);
    strcpy(name, plan.name);
    *lds_bytes = (int64_t)plan.lds_bytes;
    return 0;
}

extern "C" int mlg_rollout_selfplay_mix(const MlgEnvSpec* spec0, MlgEnvState* st, const MlgAgentDims* dims,
                                        const float* home_packed, const MlgOpponentMix* mix, MlgBatch* home,
                                        MlgBatch* away, MlgRunInfo* info, float eps_home, float eps_away,
                                        int32_t test_mode, void* stream) {
    MLG_REQUIRE(spec0 && dims && home_packed && mix && info, "rollout_selfplay_mix: null pointer");
    if (check_state(st)) return 1;
    if (check_mix_dims(spec0, dims)) return 1;
    if (check_rollout_batch(home, spec0, st, "rollout_selfplay_mix (home)") ||
        check_rollout_batch(away, spec0, st, "rollout_selfplay_mix (away)"))
        return 1;
    MLG_REQUIRE(info->ep_len && info->ret && info->won && info->draw, "rollout_selfplay_mix: run info has null tensors");
    MLG_REQUIRE(mix->packed_pool && mix->groups && mix->host_groups && mix->specs && mix->host_specs,
                "rollout_selfplay_mix: null pool / groups / specs pointer in the mixture");
    MLG_REQUIRE(mlg::aligned16(mix->packed_pool) && mlg::aligned16(home_packed),
                "rollout_selfplay_mix: packed_pool and home_packed must be 16-byte aligned");
    MLG_REQUIRE(mix->n_pool >= 1 && mix->n_specs >= 1, "rollout_selfplay_mix: n_pool=%d n_specs=%d must be >= 1",
                mix->n_pool, mix->n_specs);
    const int G = (st->B + RE - 1) / RE;
    MLG_REQUIRE(mix->n_groups == G, "rollout_selfplay_mix: n_groups=%d, B=%d envs are ceil(B / 16) = %d groups",
                mix->n_groups, st->B, G);
    for (int k = 0; k < mix->n_specs; ++k) {
        const MlgEnvSpec& s = mix->host_specs[k];
        if (check_mix_spec(&s, "specs", k)) return 1;
        MLG_REQUIRE(s.U == spec0->U, "rollout_selfplay_mix: specs[%d].U=%d differs from spec0.U=%d", k, s.U, spec0->U);
        MLG_REQUIRE(s.n_agents == spec0->n_agents, "rollout_selfplay_mix: specs[%d].n_agents=%d differs from spec0 (%d)",
                    k, s.n_agents, spec0->n_agents);
        MLG_REQUIRE(s.n_actions == spec0->n_actions, "rollout_selfplay_mix: specs[%d].n_actions differs from spec0", k);
        MLG_REQUIRE(s.grid == spec0->grid, "rollout_selfplay_mix: specs[%d].grid=%d differs from spec0 (%d)", k, s.grid,
                    spec0->grid);
        MLG_REQUIRE(s.episode_limit == spec0->episode_limit,
                    "rollout_selfplay_mix: specs[%d].episode_limit=%d differs from spec0 (%d)", k, s.episode_limit,
                    spec0->episode_limit);
        MLG_REQUIRE(s.stochastic == spec0->stochastic, "rollout_selfplay_mix: specs[%d].stochastic differs from spec0", k);
        MLG_REQUIRE(s.policy_team == spec0->policy_team, "rollout_selfplay_mix: specs[%d].policy_team differs from spec0",
                    k);
        MLG_REQUIRE(s.seed == spec0->seed, "rollout_selfplay_mix: specs[%d].seed differs from spec0", k);
    }
    for (int g = 0; g < G; ++g) {
        const MlgMixGroup& q = mix->host_groups[g];
        MLG_REQUIRE(q.away >= 0 && q.away < mix->n_pool, "rollout_selfplay_mix: groups[%d].away=%d out of the pool's "
                    "range [0, %d)", g, q.away, mix->n_pool);
        MLG_REQUIRE(q.spec >= 0 && q.spec < mix->n_specs, "rollout_selfplay_mix: groups[%d].spec=%d out of range [0, %d)",
                    g, q.spec, mix->n_specs);
    }
    MixPlan plan;
    if (int rc = plan_mix(spec0, dims, &plan)) return rc;
    const float eps0 = test_mode ? 0.f : eps_home, eps1 = test_mode ? 0.f : eps_away;
    if (plan.sn)
        return launch_rollout_sp8_mix(plan.sn, spec0, st, dims, home_packed, mix, home, away, info, eps0, eps1, test_mode,
                                      stream);
    const AgentLayout L = make_agent_layout(*dims);
    Sides sd;
    sd.bt[0] = *home;
    sd.bt[1] = *away;
    sd.P[0] = home_packed;
    sd.P[1] = nullptr;  // per workgroup, from the pool
    sd.eps[0] = eps0;
    sd.eps[1] = eps1;
    sd.ns = 2;
    sd.nh = spec0->n_agents / 2;
    MixShape sh;
    sh.U = spec0->U;
    sh.N = spec0->n_agents;
    sh.A = spec0->n_actions;
    sh.grid = spec0->grid;
    sh.episode_limit = spec0->episode_limit;
    sh.stochastic = spec0->stochastic;
    sh.policy_team = spec0->policy_team;
    sh.seed = spec0->seed;
    MixArgs mx;
    mx.pool = mix->packed_pool;
    mx.pool_stride = L.total;
    mx.groups = mix->groups;
    mx.specs = mix->specs;
    mx.n_pool = mix->n_pool;
    mx.n_specs = mix->n_specs;
    hipStream_t s = (hipStream_t)stream;
    int rc = 0;
#define MLG_MX(HH, TT) rc = launch_mix<HH, TT>(G, s, sh, *st, L, sd, mx, *info, test_mode, plan)
#define MLG_MX_H(HH)                         \
    do {                                     \
        if (plan.tpw == 1) MLG_MX(HH, 1);    \
        else if (plan.tpw == 2) MLG_MX(HH, 2); \
        else if (plan.tpw == 3) MLG_MX(HH, 3); \
        else MLG_MX(HH, 4);                  \
    } while (0)
    if (L.H == 64) MLG_MX_H(64);
    else if (L.H == 32) MLG_MX_H(32);
    else MLG_MX_H(128);
#undef MLG_MX_H
#undef MLG_MX
    if (rc) return rc;
    return mlg::check_launch("rollout_mix_kernel");
}
