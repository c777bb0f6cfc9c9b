// crossplay_device.h -- what the cross-play evaluation kernels share (crossplay.hip: DRQN, pi_logits and distinct
// policies; crossplay_ff.hip: feed-forward policies): the kernel argument blocks, the LDS carve, the env step without an
// EpisodeBatch (cp_observe / cp_env_step), the fixed-order summary reduce and the host checks of an MlgCrossplay block.
// File-local in each translation unit, like rollout_env_device.h and rollout_host.h.
#pragma once
#include <cstdlib>

#include "agent_device.h"
#include "rollout_env_device.h"
#include "rollout_host.h"

int check_agent_dims(const MlgAgentDims* d);  // agent.hip

namespace {

// What every spec of a launch agrees on (host-checked), as one kernel argument.
struct CpShape {
    int U, N, A, nh, grid, episode_limit, stochastic, policy_team;
    uint64_t seed;
};

// Dynamic-LDS carve (4-byte words). obs / avail: the current step's rows of the RE envs (obs row stride ldo floats:
// d_obs + 4, so the 16 rows of a tile start in distinct 16-byte bank slots); -1 = in the workspace instead.
struct CpLds {
    int32_t spec, x, y, hp, nhp, act, pact, prev, status, stepped, len, ret, ret2, misc, avail, obs, total;
    int32_t ldo, obs_words, avail_words;
};

__host__ __device__ inline CpLds make_cp_lds(int U, int N, int A, bool rows_in_lds) {
    CpLds r{};
    int64_t o = 0;
    const int64_t eu = (int64_t)RE * U, en = (int64_t)RE * N;
    r.spec = ro_take(o, (int64_t)(sizeof(SpecShared) / 4));
    r.x = ro_take(o, eu);
    r.y = ro_take(o, eu);
    r.hp = ro_take(o, eu);
    r.nhp = ro_take(o, eu);
    r.act = ro_take(o, eu);
    r.pact = ro_take(o, en);
    r.prev = ro_take(o, en);
    r.status = ro_take(o, RE);
    r.stepped = ro_take(o, RE);
    r.len = ro_take(o, RE);
    r.ret = ro_take(o, RE);
    r.ret2 = ro_take(o, RE);
    r.misc = ro_take(o, 4);  // [0] any env running
    r.ldo = 8 * U + 4;
    r.obs_words = (int32_t)mlg_align4(en * r.ldo);
    r.avail_words = (int32_t)mlg_align4(en * A);
    r.avail = r.obs = -1;
    if (rows_in_lds) {
        r.avail = ro_take(o, r.avail_words);
        r.obs = ro_take(o, r.obs_words);
    }
    r.total = (int32_t)o;
    return r;
}

struct CpEnv {
    int *x, *y, *hp, *nhp, *act, *pact, *prev, *status, *stepped, *len, *misc;
    float *ret, *ret2;
    float* lobs;      // [RE * N][ldo]
    int32_t* lavail;  // [RE * N][A]
    int ldo;
};

struct CpArgs {
    const float* pool;
    int64_t pool_stride;  // floats per packed policy
    const MlgCrossplayPair* pairs;
    const MlgEnvSpec* specs;
    int n_pool, n_specs, wg_per_pair, E;
    uint32_t episode0;
    int flags;  // POLICY only: bit 1 mask_before_softmax, bit 2 test_greedy (rollout_policy_kernel's flags, test mode);
                // in what was padding: the Q instantiations read their arguments where they did
    float* workspace;  // used iff the rows are not in LDS: [grid][obs_words + avail_words]
    int32_t* ep_len;
    float *ret, *ret_away;
    int32_t *won, *draw;
};

// obs / avail rows of the envs that did not finish before this step (reset: every live env; later: the envs that
// stepped, those that just terminated included -- they still receive one action).
__device__ void cp_observe(const EnvTables& T, const SpecShared& SS, const CpShape& sh, const CpEnv& R, bool stepped_only,
                           float inv_p) {
    const int tid = threadIdx.x, nthr = blockDim.x, U = sh.U, N = sh.N, A = sh.A;
    auto on = [&](int e) { return stepped_only ? R.stepped[e] != 0 : R.status[e] != 2; };
    for (int i = tid; i < RE * N * U; i += nthr) {
        const int e = i / (N * U), r = i % (N * U);
        if (!on(e)) continue;
        const int a = r / U, j = r % U;
        float o[8];
        env_obs_feat(T, R.x + e * U, R.y + e * U, R.hp + e * U, SS.aunit[a], j, inv_p, o);
        float* l = R.lobs + (e * N + a) * R.ldo + j * 8;
        *reinterpret_cast<floatx4*>(l) = floatx4{o[0], o[1], o[2], o[3]};
        *reinterpret_cast<floatx4*>(l + 4) = floatx4{o[4], o[5], o[6], o[7]};
    }
    for (int i = tid; i < RE * N * A; i += nthr) {
        const int e = i / (N * A), r = i % (N * A);
        if (!on(e)) continue;
        R.lavail[e * N * A + r] = env_avail_one(T, R.x + e * U, R.y + e * U, R.hp + e * U, SS.aunit[r / A], r % A);
    }
}

// The env phase of step t (ro_env_step of rollout.hip without the EpisodeBatch): executed actions, simultaneous
// resolution, per-env reward / termination, then the rows of t + 1. out = first result of this pair.
__device__ void cp_env_step(const EnvTables& T, const SpecShared& SS, const CpShape& sh, const CpEnv& R,
                            const CpArgs& a, int64_t out, int e0, int t, float inv_p) {
    const int tid = threadIdx.x, nthr = blockDim.x, U = sh.U, N = sh.N;
    for (int i = tid; i < RE * U; i += nthr) {
        const int e = i / U, u = i % U;
        if (R.status[e] != 0) continue;
        const int ag = SS.agent[u];
        R.act[e * U + u] = env_exec_action(T, R.x + e * U, R.y + e * U, R.hp + e * U, u,
                                           ag ? (int64_t)R.pact[e * N + ag - 1] : 0);
    }
    __syncthreads();
    for (int i = tid; i < RE * U; i += nthr) {
        const int e = i / U, j = i % U;
        if (R.status[e] != 0) continue;
        R.nhp[e * U + j] = env_resolve_hp(T, R.act + e * U, R.hp + e * U, j);
        if (R.hp[e * U + j] > 0) env_apply_move(R.act[e * U + j], &R.x[e * U + j], &R.y[e * U + j]);
    }
    __syncthreads();
    const int pt = sh.policy_team;  // team of the home side
    for (int e = tid; e < RE; e += nthr) {
        const int status = R.status[e];
        R.stepped[e] = 0;
        if (status == 2) continue;
        for (int n = 0; n < N; ++n) R.prev[e * N + n] = R.pact[e * N + n];
        if (status == 1) {  // final action taken; env done
            R.status[e] = 2;
            continue;
        }
        int alive[2] = {0, 0}, lost[2] = {0, 0}, kills[2] = {0, 0};
        for (int j = 0; j < U; ++j) {
            const int tm = SS.team[j];
            const int h0 = R.hp[e * U + j], h1 = R.nhp[e * U + j];
            if (h0 > 0) {
                lost[tm] += h0 - h1 > 0 ? h0 - h1 : 0;
                if (h1 == 0) kills[1 - tm] += 1;
            }
            if (h1 > 0) alive[tm] += 1;
            R.hp[e * U + j] = h1;
        }
        const int done = alive[0] == 0 || alive[1] == 0 || t + 1 >= sh.episode_limit;
        int won[2];
        won[0] = alive[1] == 0 && alive[0] > 0;
        won[1] = alive[0] == 0 && alive[1] > 0;
        R.ret[e] += (float)(lost[1 - pt] + 10 * kills[pt] + 200 * won[pt]) * 0.0625f;
        R.ret2[e] += (float)(lost[pt] + 10 * kills[1 - pt] + 200 * won[1 - pt]) * 0.0625f;
        R.stepped[e] = 1;
        if (done) {
            R.status[e] = 1;
            R.len[e] = t + 1;
            const int64_t b = out + e0 + e;  // e0 + e < E: envs past E start with status 2
            a.won[2 * b] = won[pt];
            a.won[2 * b + 1] = won[1 - pt];
            a.draw[b] = !won[0] && !won[1];
        }
    }
    __syncthreads();
    cp_observe(T, SS, sh, R, true, inv_p);
}

// summary[pair][8] from the per-env results, one wave per pair, in the fixed order maleague.h documents.
__global__ void __launch_bounds__(64) crossplay_summary_kernel(const int32_t* __restrict__ ep_len,
                                                              const float* __restrict__ ret,
                                                              const float* __restrict__ ret_away,
                                                              const int32_t* __restrict__ won,
                                                              const int32_t* __restrict__ draw, int E,
                                                              float* __restrict__ summary) {
    __shared__ float pf[2][64];
    __shared__ int pi[4][64];
    const int lane = threadIdx.x;
    const int64_t out = (int64_t)blockIdx.x * E;
    float r0 = 0.f, r1 = 0.f;
    int w = 0, l = 0, d = 0, len = 0;
    for (int e = lane; e < E; e += 64) {
        const int64_t b = out + e;
        const bool w0 = won[2 * b] != 0, w1 = won[2 * b + 1] != 0;
        const bool dr = draw[b] != 0 || w0 == w1;
        w += !dr && w0;
        l += !dr && !w0;
        d += dr;
        len += ep_len[b];
        r0 += ret[b];
        r1 += ret_away[b];
    }
    pf[0][lane] = r0;
    pf[1][lane] = r1;
    pi[0][lane] = w;
    pi[1][lane] = l;
    pi[2][lane] = d;
    pi[3][lane] = len;
    __syncthreads();
    if (lane != 0) return;
    float s0 = 0.f, s1 = 0.f;
    int sw = 0, sl = 0, sd = 0, slen = 0;
    for (int k = 0; k < 64; ++k) {
        s0 += pf[0][k];
        s1 += pf[1][k];
        sw += pi[0][k];
        sl += pi[1][k];
        sd += pi[2][k];
        slen += pi[3][k];
    }
    float* o = summary + (int64_t)blockIdx.x * 8;
    o[0] = (float)E;
    o[1] = (float)sw;
    o[2] = (float)sl;
    o[3] = (float)sd;
    o[4] = s0;
    o[5] = s1;
    o[6] = (float)slen;
    o[7] = 0.f;
}

bool rows_forced_to_workspace() {
    const char* v = getenv("MLG_CROSSPLAY_OBS_WORKSPACE");
    return v && v[0] == '1';
}

// The LDS carve of a launch: rows in LDS when they fit, else in the workspace.
CpLds pick_cp_lds(int U, int N, int A) {
    const CpLds in = make_cp_lds(U, N, A, true);
    if ((int64_t)in.total * 4 <= LDS_LIMIT_BYTES && !rows_forced_to_workspace()) return in;
    return make_cp_lds(U, N, A, false);
}

int check_crossplay_dims(const MlgAgentDims* d) {
    if (check_agent_dims(d)) return 1;
    MLG_REQUIRE(d->d_obs % 8 == 0 && d->d_obs / 8 >= 2 && d->d_obs / 8 <= MLG_MAXU,
                "crossplay: d_obs=%d is not 8 * U with U in [2, %d]", d->d_obs, MLG_MAXU);
    MLG_REQUIRE(2 * d->n_agents <= d->d_obs / 8, "crossplay: n_agents=%d per side exceeds U / 2 = %d", d->n_agents,
                d->d_obs / 16);
    return 0;
}

// The workspace need of a launch (mlg_crossplay_workspace_floats and its feed-forward twin); -1 on bad arguments.
int64_t cp_workspace_floats(const MlgAgentDims* dims, int32_t n_pairs, int32_t E) {
    if (check_crossplay_dims(dims)) return -1;
    if (n_pairs < 1 || E < 1) {
        mlg::fail("crossplay: n_pairs=%d and E=%d must be >= 1", n_pairs, E);
        return -1;
    }
    const CpLds lay = pick_cp_lds(dims->d_obs / 8, 2 * dims->n_agents, dims->n_actions);
    if (lay.obs >= 0) return 4;  // rows in LDS: nothing but a valid pointer is needed
    const int64_t grid = (int64_t)n_pairs * ((E + RE - 1) / RE);
    return grid * ((int64_t)lay.obs_words + lay.avail_words);
}

// What the host checks of an MlgCrossplay block leave for the launch.
struct CpLaunch {
    CpArgs a;
    CpShape sh;
    CpLds lay;
    int grid, threads, tpw;
};

// The checks of an MlgCrossplay block (after check_crossplay_dims) and the kernel arguments. L: the layout of one packed
// block (its total is the pool's row stride); max_at: the pi_logits pick's bound on action tiles (0: none); distinct:
// one tile per agent of either side instead of 16 rows of (env, agent).
int cp_prepare(const MlgAgentDims* dims, const MlgCrossplay* c, const AgentLayout& L, int max_at, int flags,
               bool distinct, CpLaunch* out) {
    MLG_REQUIRE(c != nullptr, "crossplay: null argument block");
    MLG_REQUIRE(c->packed_pool && c->pairs && c->host_pairs && c->specs && c->host_specs && c->workspace,
                "crossplay: null pool / pairs / specs / workspace pointer");
    MLG_REQUIRE(c->ep_len && c->ret && c->ret_away && c->won && c->draw && c->summary, "crossplay: null output pointer");
    MLG_REQUIRE(mlg::aligned16(c->packed_pool) && mlg::aligned16(c->workspace),
                "crossplay: packed_pool and workspace must be 16-byte aligned");
    MLG_REQUIRE(c->n_pool >= 1 && c->n_pairs >= 1 && c->n_specs >= 1 && c->E >= 1,
                "crossplay: n_pool=%d n_pairs=%d n_specs=%d E=%d must all be >= 1", c->n_pool, c->n_pairs, c->n_specs,
                c->E);
    const MlgEnvSpec& s0 = c->host_specs[0];
    for (int k = 0; k < c->n_specs; ++k) {
        const MlgEnvSpec& s = c->host_specs[k];
        if (check_spec(&s)) return 1;
        MLG_REQUIRE(s.n_policy_teams == 2 && s.n_agents % 2 == 0,
                    "crossplay: specs[%d] has n_policy_teams=%d with %d agents; evaluation needs the symmetric "
                    "two-policy-team scenario", k, s.n_policy_teams, s.n_agents);
        MLG_REQUIRE(s.U == s0.U, "crossplay: specs[%d].U=%d differs from specs[0].U=%d", k, s.U, s0.U);
        MLG_REQUIRE(s.n_agents == s0.n_agents, "crossplay: specs[%d].n_agents=%d differs from specs[0] (%d)", k,
                    s.n_agents, s0.n_agents);
        MLG_REQUIRE(s.n_actions == s0.n_actions, "crossplay: specs[%d].n_actions differs from specs[0]", k);
        MLG_REQUIRE(s.grid == s0.grid, "crossplay: specs[%d].grid=%d differs from specs[0] (%d)", k, s.grid, s0.grid);
        MLG_REQUIRE(s.episode_limit == s0.episode_limit, "crossplay: specs[%d].episode_limit=%d differs from specs[0] (%d)",
                    k, s.episode_limit, s0.episode_limit);
        MLG_REQUIRE(s.stochastic == s0.stochastic, "crossplay: specs[%d].stochastic differs from specs[0]", k);
        MLG_REQUIRE(s.policy_team == s0.policy_team, "crossplay: specs[%d].policy_team differs from specs[0]", k);
        MLG_REQUIRE(s.seed == s0.seed, "crossplay: specs[%d].seed differs from specs[0]", k);
        const int nh = s.n_agents / 2;
        for (int a = 0; a < nh; ++a)
            MLG_REQUIRE(s.team[s.agent_unit[a]] == s.policy_team && s.team[s.agent_unit[nh + a]] == 1 - s.policy_team,
                        "crossplay: specs[%d]: agents 0..%d must be the home team, %d..%d the away team", k, nh - 1, nh,
                        2 * nh - 1);
    }
    const int nh = s0.n_agents / 2;
    MLG_REQUIRE(dims->n_agents == nh && dims->n_actions == s0.n_actions && dims->d_obs == 8 * s0.U,
                "crossplay: agent dims do not match one side of the env (N=%d/%d A=%d/%d d_obs=%d/%d)", dims->n_agents,
                nh, dims->n_actions, s0.n_actions, dims->d_obs, 8 * s0.U);
    for (int k = 0; k < c->n_pairs; ++k) {
        const MlgCrossplayPair& p = c->host_pairs[k];
        MLG_REQUIRE(p.home >= 0 && p.home < c->n_pool && p.away >= 0 && p.away < c->n_pool,
                    "crossplay: pairs[%d] = (home %d, away %d) out of the pool's range [0, %d)", k, p.home, p.away,
                    c->n_pool);
        MLG_REQUIRE(p.spec >= 0 && p.spec < c->n_specs, "crossplay: pairs[%d].spec=%d out of range [0, %d)", k, p.spec,
                    c->n_specs);
    }
    const int wg_per_pair = (c->E + RE - 1) / RE;
    const int64_t grid64 = (int64_t)c->n_pairs * wg_per_pair;
    MLG_REQUIRE(grid64 <= 0x7fffffff && (int64_t)c->n_pairs * c->E <= 0x3fffffff,
                "crossplay: n_pairs=%d x E=%d is too large for one launch", c->n_pairs, c->E);
    MLG_REQUIRE(!max_at || L.Ap <= 16 * max_at, "crossplay: n_actions=%d does not fit %d action tiles (policy pick)",
                dims->n_actions, max_at);
    const int tiles = distinct ? 2 * nh : 2 * ((RE * nh + 15) / 16);  // distinct: one tile per agent of either side
    const int W = tiles < 8 ? tiles : 8;
    const int tpw = (tiles + W - 1) / W;
    MLG_REQUIRE(tpw <= 4, "crossplay: n_agents=%d per side needs %d agent tiles per wave > 4", nh, tpw);
    const CpLds lay = pick_cp_lds(s0.U, s0.n_agents, s0.n_actions);
    MLG_REQUIRE((int64_t)lay.total * 4 <= LDS_LIMIT_BYTES, "crossplay: U=%d needs %d B of LDS", s0.U, lay.total * 4);
    const int64_t ws_need = lay.obs >= 0 ? 4 : grid64 * ((int64_t)lay.obs_words + lay.avail_words);
    MLG_REQUIRE(c->workspace_floats >= ws_need, "crossplay: workspace of %lld floats, the launch needs %lld "
                "(mlg_crossplay_workspace_floats)", (long long)c->workspace_floats, (long long)ws_need);

    CpArgs& a = out->a;
    a.pool = c->packed_pool;
    a.pool_stride = L.total;
    a.pairs = c->pairs;
    a.specs = c->specs;
    a.n_pool = c->n_pool;
    a.n_specs = c->n_specs;
    a.wg_per_pair = wg_per_pair;
    a.E = c->E;
    a.episode0 = c->episode0;
    a.workspace = c->workspace;
    a.ep_len = c->ep_len;
    a.ret = c->ret;
    a.ret_away = c->ret_away;
    a.won = c->won;
    a.draw = c->draw;
    a.flags = flags;
    CpShape& sh = out->sh;
    sh.U = s0.U;
    sh.N = s0.n_agents;
    sh.A = s0.n_actions;
    sh.nh = nh;
    sh.grid = s0.grid;
    sh.episode_limit = s0.episode_limit;
    sh.stochastic = s0.stochastic;
    sh.policy_team = s0.policy_team;
    sh.seed = s0.seed;
    out->lay = lay;
    out->grid = (int)grid64;
    out->threads = W * 64;
    out->tpw = tpw;
    return 0;
}

// The second kernel of every cross-play call.
int cp_launch_summary(const MlgCrossplay* c, hipStream_t s) {
    hipLaunchKernelGGL(crossplay_summary_kernel, dim3(c->n_pairs), dim3(64), 0, s, c->ep_len, c->ret, c->ret_away, c->won,
                       c->draw, c->E, c->summary);
    return mlg::check_launch("crossplay_summary_kernel");
}

}  // namespace
