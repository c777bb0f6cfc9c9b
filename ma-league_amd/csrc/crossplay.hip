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
// from rollout_host.h (shared with rollout.hip). The argument blocks, the LDS carve, cp_observe / cp_env_step (the env
// step without an EpisodeBatch), the summary kernel and the checks of an MlgCrossplay block are crossplay_device.h's,
// shared with crossplay_ff.hip.
#include <cstdlib>

#include "agent_device.h"
#include "coma_device.h"
#include "crossplay_device.h"

namespace {

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
    return cp_workspace_floats(dims, n_pairs, E);
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
    const AgentLayout L = make_agent_layout(*dims);
    CpLaunch cl;
    if (int rc = cp_prepare(dims, c, L, policy ? RO_MAXAT : 0, flags, distinct, &cl)) return rc;
    const CpArgs& a = cl.a;
    const CpShape& sh = cl.sh;
    const CpLds& lay = cl.lay;
    hipStream_t s = (hipStream_t)stream;
    const int grid = cl.grid, threads = cl.threads, tpw = cl.tpw;
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
    return cp_launch_summary(c, s);
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
