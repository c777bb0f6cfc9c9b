// crossplay.hip -- league cross-play evaluation: every (home policy, away policy, roster) pair in one launch.
//
// Joint-policy-correlation evaluation (src/runs/evaluation/jpc_eval_run.py:62-89) needs E greedy games for each of
// P x P policy pairs. The training rollout plays one pair per launch and writes two [B][T1] EpisodeBatches nobody
// reads; this kernel exists only to evaluate: a workgroup owns RE = 16 envs of ONE pair, reads its two policies from
// the packed pool by index and its roster from a device array of specs, keeps the obs / avail rows of the current
// step on chip (LDS; a per-workgroup workspace slice when one step of 16 envs does not fit) and writes per-env
// results only. Nothing scales with episode_limit.
//
// The arithmetic is the generic fp32 self-play kernel's (rollout_kernel<H, TPW, false> with two sides, test mode):
// same tile layout (side s owns tiles [s tps, (s + 1) tps), row r = env r / nh, agent s nh + r % nh), same MFMA cell
// (agent_cell_hidden / agent_q_tile / argmax_*) in the same order, same env step. Env (pair k, episode e) runs as env
// index e with episode counter episode0, so the results are bit-identical to one mlg_rollout_selfplay per pair.
//
// mlg_crossplay_rollout_policy plays pi_logits policies (COMA): the POLICY = true instantiation of the same kernel, whose
// pick is rollout_policy.hip's test-mode selection (ro_policy_select, coma_device.h) -- the first-index argmax of the
// masked probabilities, or a draw from the floor-less probabilities on the counter RNG with episode0 as the episode
// counter. Its per-env results are bit-identical to one test-mode mlg_rollout_selfplay_policy per pair on the global
// arm.
//
// RE, SpecShared, load_spec_tables and ro_take come from rollout_env_device.h, check_spec, LDS_LIMIT_BYTES and allow_lds
// from rollout_host.h (shared with rollout.hip). cp_observe / cp_env_step are this file's own: the env step without an
// EpisodeBatch.
#include <cstdlib>

#include "agent_device.h"
#include "coma_device.h"
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

template <int H, int TPW, bool POLICY = false>
__global__ void __launch_bounds__(512) crossplay_kernel(CpArgs a, CpShape sh, AgentLayout L, CpLds lay) {
    constexpr int HC = H / 16;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, W = nthr >> 6;
    const int pair = blockIdx.x / a.wg_per_pair, e0 = (blockIdx.x % a.wg_per_pair) * RE;
    const int64_t out = (int64_t)pair * a.E;
    const MlgCrossplayPair pr = a.pairs[pair];
    const int U = sh.U, N = sh.N, A = sh.A, nh = sh.nh;
    // The host validated its copy of the pair table; the launch reads the caller's device copy. A device row that is
    // out of range plays nothing (ep_len -1) instead of reading past the pool or the spec array.
    if ((unsigned)pr.home >= (unsigned)a.n_pool || (unsigned)pr.away >= (unsigned)a.n_pool ||
        (unsigned)pr.spec >= (unsigned)a.n_specs) {
        for (int e = tid; e < RE; e += nthr) {
            if (e0 + e >= a.E) continue;
            const int64_t b = out + e0 + e;
            a.ep_len[b] = -1;
            a.ret[b] = 0.f;
            a.ret_away[b] = 0.f;
            a.won[2 * b] = a.won[2 * b + 1] = 0;
            a.draw[b] = 0;
        }
        return;
    }
    SpecShared& SS = *reinterpret_cast<SpecShared*>(smem + lay.spec);
    CpEnv R;
    R.x = smem + lay.x;
    R.y = smem + lay.y;
    R.hp = smem + lay.hp;
    R.nhp = smem + lay.nhp;
    R.act = smem + lay.act;
    R.pact = smem + lay.pact;
    R.prev = smem + lay.prev;
    R.status = smem + lay.status;
    R.stepped = smem + lay.stepped;
    R.len = smem + lay.len;
    R.misc = smem + lay.misc;
    R.ret = reinterpret_cast<float*>(smem + lay.ret);
    R.ret2 = reinterpret_cast<float*>(smem + lay.ret2);
    R.ldo = lay.ldo;
    if (lay.obs >= 0) {
        R.lobs = reinterpret_cast<float*>(smem + lay.obs);
        R.lavail = smem + lay.avail;
    } else {  // one step of this workgroup's rows in its workspace slice (written and read by this workgroup only)
        float* ws = a.workspace + (int64_t)blockIdx.x * (lay.obs_words + lay.avail_words);
        R.lobs = ws;
        R.lavail = reinterpret_cast<int32_t*>(ws + lay.obs_words);
    }
    load_spec_tables(a.specs[pr.spec], SS);  // the pair's roster, from device memory
    EnvTables T;
    T.team = SS.team;
    T.role = SS.role;
    T.melee = SS.melee;
    T.agent = SS.agent;
    T.U = U;
    T.grid = sh.grid;
    T.episode_limit = sh.episode_limit;
    T.stochastic = sh.stochastic;
    const float inv_p = 1.0f / (float)pow2_at_least(sh.grid);
    const float* P0 = a.pool + (int64_t)pr.home * a.pool_stride;
    const float* P1 = a.pool + (int64_t)pr.away * a.pool_stride;

    // ---- reset: env (pair, e) = env index e0 + e, episode counter episode0 ----
    for (int e = tid; e < RE; e += nthr) {
        R.len[e] = 0;
        R.ret[e] = 0.f;
        R.ret2[e] = 0.f;
        R.stepped[e] = 0;
        R.status[e] = e0 + e < a.E ? 0 : 2;
    }
    __syncthreads();
    for (int i = tid; i < RE * U; i += nthr) {
        const int e = i / U, u = i % U;
        if (R.status[e] == 2) continue;
        const int tm = SS.team[u];
        env_spawn_unit(T, mlg_env_key(sh.seed, e0 + e), a.episode0, u, SS.team_first[tm], SS.team_size[tm], R.x + e * U,
                       R.y + e * U, R.hp + e * U);
    }
    __syncthreads();
    cp_observe(T, SS, sh, R, false, inv_p);
    __syncthreads();

    floatx4 h[TPW][HC];
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
        for (int c = 0; c < HC; ++c) h[ti][c] = floatx4{0.f, 0.f, 0.f, 0.f};
    const int tps = (RE * nh + 15) / 16, n_tiles = 2 * tps;
    const int col = lane & 15, g = lane >> 4;
    const int n_at = L.Ap / 16;
    const int T1 = sh.episode_limit + 1;
    for (int t = 0; t < T1; ++t) {
        // ---- agent phase: rows of envs with status 0 (running) or 1 (final action), greedy ----
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti) {
            const int tile = wave + ti * W;
            if (tile >= n_tiles) continue;
            const int side = tile >= tps;
            const int r = (tile - side * tps) * 16 + col;
            const bool in_range = r < RE * nh;
            const int e = in_range ? r / nh : 0, ln = r % nh, ag = side * nh + ln;
            const bool valid = in_range && R.status[e] < 2;
            if (!__any(valid)) continue;  // wave-uniform skip of finished tiles
            // opaque zero offset per tile: keeps t- and tile-invariant weight loads out of (spilled) registers
            int zero = 0;
            asm volatile("" : "+s"(zero));
            const WView Wv = global_view((side ? P1 : P0) + zero, L);
            RowIn in;
            in.x = valid ? R.lobs + (e * N + ag) * R.ldo : nullptr;
            in.onehot = nullptr;
            in.prev_action = (valid && t > 0) ? R.prev[e * N + ag] : -1;
            in.agent = valid ? ln : 0;
            agent_cell_hidden<H>(Wv, L, in, h[ti], lane);
            const int32_t* av = valid ? R.lavail + (e * N + ag) * A : nullptr;
            int act;
            if constexpr (POLICY) {  // rollout_policy_kernel's selection site in test mode
                floatx4 qt[RO_MAXAT];
#pragma unroll
                for (int at = 0; at < RO_MAXAT; ++at)
                    qt[at] = at < n_at ? agent_q_tile<H>(Wv, h[ti], at, lane) : floatx4{0.f, 0.f, 0.f, 0.f};
                const bool greedy = (a.flags & 4) != 0;
                float u = 0.f;
                if (valid && !greedy)
                    u = mlg_u01(mlg_rng(mlg_env_key(sh.seed, e0 + e),
                                        mlg_ctr(a.episode0, (uint32_t)t, MLG_PURPOSE_POLICY, (uint32_t)ag)));
                act = ro_policy_select(qt, n_at, av, A, lane, 0.f, (a.flags & 2) != 0, true, greedy, u);
            } else {
                ArgmaxState as{-INFINITY, 1 << 30};
                for (int at = 0; at < n_at; ++at) {
                    const floatx4 q = agent_q_tile<H>(Wv, h[ti], at, lane);
                    argmax_accumulate(as, q, av, at, A, lane);
                }
                act = argmax_reduce(as);
            }
            if (valid && g == 0) R.pact[e * N + ag] = act;
        }
        __syncthreads();
        cp_env_step(T, SS, sh, R, a, out, e0, t, inv_p);
        if (tid == 0) {
            int n = 0;
            for (int e = 0; e < RE; ++e) n += R.status[e] < 2;
            R.misc[0] = n > 0;
        }
        __syncthreads();
        if (!R.misc[0]) break;
    }
    for (int e = tid; e < RE; e += nthr) {
        if (e0 + e >= a.E) continue;
        const int64_t b = out + e0 + e;
        a.ep_len[b] = R.len[e];
        a.ret[b] = R.ret[e];
        a.ret_away[b] = R.ret2[e];
    }
}

// mlg_crossplay_rollout_distinct: policies with one DRQN per agent slot (mac: distinct). The pool holds n_pool * nh
// blocks, policy p being blocks [p nh, (p + 1) nh). The body is crossplay_kernel's Q instantiation with the agent
// phase agent-major, as rollout_selfplay_distinct_kernel's (distinct_selfplay.hip): tile a = s nh + ln is agent ln of
// side s across the workgroup's 16 envs (column = env), 2 nh tiles, wave w owns tiles w, w + W, ...; the weight view
// of a tile is wave-uniform. The obs / avail rows (LDS or the workspace slice) are read by column = env. Env (pair k,
// episode e) is bit-identical to env e of one test-mode mlg_rollout_selfplay_distinct of that pair with episode
// counter episode0. A kernel of its own, not a template flag of crossplay_kernel, for the reason rollout_policy.hip
// records.
template <int H, int TPW>
__global__ void __launch_bounds__(512) crossplay_distinct_kernel(CpArgs a, CpShape sh, AgentLayout L, CpLds lay) {
    constexpr int HC = H / 16;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), W = nthr >> 6;
    const int pair = blockIdx.x / a.wg_per_pair, e0 = (blockIdx.x % a.wg_per_pair) * RE;
    const int64_t out = (int64_t)pair * a.E;
    const MlgCrossplayPair pr = a.pairs[pair];
    const int U = sh.U, N = sh.N, A = sh.A, nh = sh.nh;
    // As crossplay_kernel: a device pair row that is out of range plays nothing (ep_len -1).
    if ((unsigned)pr.home >= (unsigned)a.n_pool || (unsigned)pr.away >= (unsigned)a.n_pool ||
        (unsigned)pr.spec >= (unsigned)a.n_specs) {
        for (int e = tid; e < RE; e += nthr) {
            if (e0 + e >= a.E) continue;
            const int64_t b = out + e0 + e;
            a.ep_len[b] = -1;
            a.ret[b] = 0.f;
            a.ret_away[b] = 0.f;
            a.won[2 * b] = a.won[2 * b + 1] = 0;
            a.draw[b] = 0;
        }
        return;
    }
    SpecShared& SS = *reinterpret_cast<SpecShared*>(smem + lay.spec);
    CpEnv R;
    R.x = smem + lay.x;
    R.y = smem + lay.y;
    R.hp = smem + lay.hp;
    R.nhp = smem + lay.nhp;
    R.act = smem + lay.act;
    R.pact = smem + lay.pact;
    R.prev = smem + lay.prev;
    R.status = smem + lay.status;
    R.stepped = smem + lay.stepped;
    R.len = smem + lay.len;
    R.misc = smem + lay.misc;
    R.ret = reinterpret_cast<float*>(smem + lay.ret);
    R.ret2 = reinterpret_cast<float*>(smem + lay.ret2);
    R.ldo = lay.ldo;
    if (lay.obs >= 0) {
        R.lobs = reinterpret_cast<float*>(smem + lay.obs);
        R.lavail = smem + lay.avail;
    } else {  // one step of this workgroup's rows in its workspace slice (written and read by this workgroup only)
        float* ws = a.workspace + (int64_t)blockIdx.x * (lay.obs_words + lay.avail_words);
        R.lobs = ws;
        R.lavail = reinterpret_cast<int32_t*>(ws + lay.obs_words);
    }
    load_spec_tables(a.specs[pr.spec], SS);  // the pair's roster, from device memory
    EnvTables T;
    T.team = SS.team;
    T.role = SS.role;
    T.melee = SS.melee;
    T.agent = SS.agent;
    T.U = U;
    T.grid = sh.grid;
    T.episode_limit = sh.episode_limit;
    T.stochastic = sh.stochastic;
    const float inv_p = 1.0f / (float)pow2_at_least(sh.grid);
    // policy p = blocks [p nh, (p + 1) nh) of the pool
    const float* P0 = a.pool + (int64_t)pr.home * nh * a.pool_stride;
    const float* P1 = a.pool + (int64_t)pr.away * nh * a.pool_stride;

    // ---- reset: env (pair, e) = env index e0 + e, episode counter episode0 ----
    for (int e = tid; e < RE; e += nthr) {
        R.len[e] = 0;
        R.ret[e] = 0.f;
        R.ret2[e] = 0.f;
        R.stepped[e] = 0;
        R.status[e] = e0 + e < a.E ? 0 : 2;
    }
    __syncthreads();
    for (int i = tid; i < RE * U; i += nthr) {
        const int e = i / U, u = i % U;
        if (R.status[e] == 2) continue;
        const int tm = SS.team[u];
        env_spawn_unit(T, mlg_env_key(sh.seed, e0 + e), a.episode0, u, SS.team_first[tm], SS.team_size[tm], R.x + e * U,
                       R.y + e * U, R.hp + e * U);
    }
    __syncthreads();
    cp_observe(T, SS, sh, R, false, inv_p);
    __syncthreads();

    floatx4 h[TPW][HC];
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
        for (int c = 0; c < HC; ++c) h[ti][c] = floatx4{0.f, 0.f, 0.f, 0.f};
    const int e = lane & 15, g = lane >> 4;  // column = env of the workgroup
    const int n_at = L.Ap / 16;
    const int T1 = sh.episode_limit + 1;
    for (int t = 0; t < T1; ++t) {
        // ---- agent phase: tile ag = agent ln of side s in the envs with status 0 or 1, greedy ----
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti) {
            const int ag = wave + ti * W;  // the tile's global agent index s nh + ln: wave-uniform
            if (ag >= N) continue;
            const int side = ag >= nh, ln = ag - side * nh;
            const bool valid = R.status[e] < 2;  // envs past E carry status 2 from the reset
            if (!__any(valid)) continue;  // wave-uniform skip once every env is done
            // opaque zero offset per tile: keeps t- and tile-invariant weight loads out of (spilled) registers
            int zero = 0;
            asm volatile("" : "+s"(zero));
            const WView Wv = global_view((side ? P1 : P0) + (int64_t)ln * a.pool_stride + zero, L);
            RowIn in;
            in.x = valid ? R.lobs + (e * N + ag) * R.ldo : nullptr;
            in.onehot = nullptr;
            in.prev_action = (valid && t > 0) ? R.prev[e * N + ag] : -1;
            in.agent = 0;
            agent_cell_hidden<H>(Wv, L, in, h[ti], lane);
            const int32_t* av = valid ? R.lavail + (e * N + ag) * A : nullptr;
            ArgmaxState as{-INFINITY, 1 << 30};
            for (int at = 0; at < n_at; ++at) {
                const floatx4 q = agent_q_tile<H>(Wv, h[ti], at, lane);
                argmax_accumulate(as, q, av, at, A, lane);
            }
            const int act = argmax_reduce(as);
            if (valid && g == 0) R.pact[e * N + ag] = act;
        }
        __syncthreads();
        cp_env_step(T, SS, sh, R, a, out, e0, t, inv_p);
        if (tid == 0) {
            int n = 0;
            for (int x = 0; x < RE; ++x) n += R.status[x] < 2;
            R.misc[0] = n > 0;
        }
        __syncthreads();
        if (!R.misc[0]) break;
    }
    for (int x = tid; x < RE; x += nthr) {
        if (e0 + x >= a.E) continue;
        const int64_t b = out + e0 + x;
        a.ep_len[b] = R.len[x];
        a.ret[b] = R.ret[x];
        a.ret_away[b] = R.ret2[x];
    }
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

__global__ void pack_agent_pool_kernel(AgentLayout L, const float* __restrict__ flat, int64_t row_stride,
                                       float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.total) return;
    const float* f = flat + (int64_t)blockIdx.y * row_stride;
    const int64_t H = L.H;
    MlgAgentParams p;  // named_parameters() order (AGENT_ORDER of learners/q_learner.py)
    p.fc1_w = f;
    p.fc1_b = p.fc1_w + H * L.d_in;
    p.w_ih = p.fc1_b + H;
    p.w_hh = p.w_ih + 3 * H * H;
    p.b_ih = p.w_hh + 3 * H * H;
    p.b_hh = p.b_ih + 3 * H;
    p.fc2_w = p.b_hh + 3 * H;
    p.fc2_b = p.fc2_w + (int64_t)L.A * H;
    out[(int64_t)blockIdx.y * L.total + i] = pack_agent_elem(L, p, i);
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

template <int H, int TPW, bool POLICY>
int launch_crossplay(int grid, int threads, hipStream_t s, const CpArgs& a, const CpShape& sh, const AgentLayout& L,
                     const CpLds& lay) {
    const size_t bytes = (size_t)lay.total * 4;
    auto kern = crossplay_kernel<H, TPW, POLICY>;
    if (int rc = allow_lds(kern, bytes, "crossplay")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), bytes, s, a, sh, L, lay);
    return 0;
}

template <int H, int TPW>
int launch_crossplay_distinct(int grid, int threads, hipStream_t s, const CpArgs& a, const CpShape& sh,
                              const AgentLayout& L, const CpLds& lay) {
    const size_t bytes = (size_t)lay.total * 4;
    auto kern = crossplay_distinct_kernel<H, TPW>;
    if (int rc = allow_lds(kern, bytes, "crossplay_distinct")) return rc;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), bytes, s, a, sh, L, lay);
    return 0;
}

int crossplay_rollout(const MlgAgentDims* dims, const MlgCrossplay* c, bool policy, int flags, void* stream,
                      bool distinct = false);

}  // namespace

extern "C" int64_t mlg_crossplay_workspace_floats(const MlgAgentDims* dims, int32_t n_pairs, int32_t E) {
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

extern "C" int mlg_crossplay_rollout(const MlgAgentDims* dims, const MlgCrossplay* c, void* stream) {
    return crossplay_rollout(dims, c, false, 0, stream);
}

extern "C" int mlg_crossplay_rollout_policy(const MlgAgentDims* dims, const MlgCrossplay* c,
                                            int32_t mask_before_softmax, int32_t test_greedy, void* stream) {
    return crossplay_rollout(dims, c, true, (mask_before_softmax ? 2 : 0) | (test_greedy ? 4 : 0), stream);
}

// Distinct per-agent networks: c->packed_pool holds c->n_pool * dims->n_agents blocks, policy p being blocks
// [p nh, (p + 1) nh); everything else is mlg_crossplay_rollout's. The workspace need is mlg_crossplay_workspace_floats'.
extern "C" int mlg_crossplay_rollout_distinct(const MlgAgentDims* dims, const MlgCrossplay* c, void* stream) {
    return crossplay_rollout(dims, c, false, 0, stream, true);
}

namespace {

// The entry points: the checks, the launch of crossplay_kernel<H, TPW, policy> (distinct: of
// crossplay_distinct_kernel<H, TPW>) and the summary.
int crossplay_rollout(const MlgAgentDims* dims, const MlgCrossplay* c, bool policy, int flags, void* stream,
                      bool distinct) {
    if (check_crossplay_dims(dims)) return 1;
    MLG_REQUIRE(!distinct || dims->obs_agent_id == 0,
                "crossplay_distinct: obs_agent_id must be 0 (distinct agent networks take no agent id: network i is "
                "agent i)");
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
    const AgentLayout L = make_agent_layout(*dims);
    MLG_REQUIRE(!policy || L.Ap <= 16 * RO_MAXAT, "crossplay: n_actions=%d does not fit %d action tiles (policy pick)",
                dims->n_actions, RO_MAXAT);
    const int tiles = distinct ? 2 * nh : 2 * ((RE * nh + 15) / 16);  // distinct: one tile per agent of either side
    const int W = tiles < 8 ? tiles : 8;
    const int tpw = (tiles + W - 1) / W;
    MLG_REQUIRE(tpw <= 4, "crossplay: n_agents=%d per side needs %d agent tiles per wave > 4", nh, tpw);
    const CpLds lay = pick_cp_lds(s0.U, s0.n_agents, s0.n_actions);
    MLG_REQUIRE((int64_t)lay.total * 4 <= LDS_LIMIT_BYTES, "crossplay: U=%d needs %d B of LDS", s0.U, lay.total * 4);
    const int64_t ws_need = lay.obs >= 0 ? 4 : grid64 * ((int64_t)lay.obs_words + lay.avail_words);
    MLG_REQUIRE(c->workspace_floats >= ws_need, "crossplay: workspace of %lld floats, the launch needs %lld "
                "(mlg_crossplay_workspace_floats)", (long long)c->workspace_floats, (long long)ws_need);

    CpArgs a;
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
    CpShape sh;
    sh.U = s0.U;
    sh.N = s0.n_agents;
    sh.A = s0.n_actions;
    sh.nh = nh;
    sh.grid = s0.grid;
    sh.episode_limit = s0.episode_limit;
    sh.stochastic = s0.stochastic;
    sh.policy_team = s0.policy_team;
    sh.seed = s0.seed;
    hipStream_t s = (hipStream_t)stream;
    const int grid = (int)grid64, threads = W * 64;
    int rc = 0;
#define MLG_CP(HH, TT)                                                                           \
    rc = distinct ? launch_crossplay_distinct<HH, TT>(grid, threads, s, a, sh, L, lay)           \
         : policy ? launch_crossplay<HH, TT, true>(grid, threads, s, a, sh, L, lay)              \
                  : launch_crossplay<HH, TT, false>(grid, threads, s, a, sh, L, lay)
#define MLG_CP_H(HH)                   \
    do {                               \
        if (tpw == 1) MLG_CP(HH, 1);   \
        else if (tpw == 2) MLG_CP(HH, 2); \
        else if (tpw == 3) MLG_CP(HH, 3); \
        else MLG_CP(HH, 4);            \
    } while (0)
    if (L.H == 64) MLG_CP_H(64);
    else if (L.H == 32) MLG_CP_H(32);
    else if (L.H == 128) MLG_CP_H(128);
    else return mlg::fail("crossplay: rnn_hidden_dim=%d unsupported (32, 64, 128)", L.H);
#undef MLG_CP_H
#undef MLG_CP
    if (rc) return rc;
    if (mlg::check_launch(distinct ? "crossplay_distinct_kernel" : "crossplay_kernel")) return 1;
    hipLaunchKernelGGL(crossplay_summary_kernel, dim3(c->n_pairs), dim3(64), 0, s, c->ep_len, c->ret, c->ret_away, c->won,
                       c->draw, c->E, c->summary);
    return mlg::check_launch("crossplay_summary_kernel");
}

}  // namespace

extern "C" int mlg_pack_agent_pool(const MlgAgentDims* dims, const float* flat, int64_t row_stride, int32_t P,
                                   float* packed_pool, void* stream) {
    if (check_agent_dims(dims)) return 1;
    MLG_REQUIRE(flat && packed_pool && P >= 1 && P <= 65535, "pack_agent_pool: bad arguments (P=%d)", P);
    const AgentLayout L = make_agent_layout(*dims);
    const int64_t H = L.H;
    const int64_t n_params = H * L.d_in + H + 6 * H * H + 6 * H + (int64_t)L.A * H + L.A;
    MLG_REQUIRE(row_stride >= n_params, "pack_agent_pool: row_stride=%lld < %lld parameters of the agent",
                (long long)row_stride, (long long)n_params);
    hipLaunchKernelGGL(pack_agent_pool_kernel, dim3((unsigned)((L.total + 255) / 256), (unsigned)P), dim3(256), 0,
                       (hipStream_t)stream, L, flat, row_stride, packed_pool);
    return mlg::check_launch("pack_agent_pool_kernel");
}
