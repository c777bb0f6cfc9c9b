// crossplay_ff.hip -- league cross-play evaluation for feed-forward policies (agent: dqn): mlg_crossplay_rollout_ff, and
// the pool packing that feeds it: mlg_ff_pack_pool.
//
// crossplay_kernel's Q instantiation (crossplay.hip) with the agent phase of rollout_ff_selfplay_kernel
// (rollout_ff_selfplay.hip) in test mode: ff_hidden -> agent_q_tile per action tile -> masked first-index argmax, no
// hidden state carried, weights read from global memory. Same tile layout (side s owns tiles [s tps, (s + 1) tps), row
// r = env r / nh, agent s nh + r % nh), same env step (cp_observe / cp_env_step of crossplay_device.h). Env (pair k,
// episode e) runs as env index e with episode counter episode0, so the per-env results are bit-identical to one
// test-mode mlg_rollout_selfplay_ff per pair. A kernel of its own, not a template flag of crossplay_kernel, for the
// reason rollout_policy.hip records.
#include "agent_ff_device.h"
#include "crossplay_device.h"

namespace {

template <int H, int TPW>
__global__ void __launch_bounds__(512) crossplay_ff_kernel(CpArgs a, CpShape sh, AgentLayout L, CpLds lay) {
    constexpr int HC = H / 16;
    extern __shared__ __attribute__((aligned(16))) int smem[];
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int lane = tid & 63, wave = tid >> 6, W = nthr >> 6;
    const int pair = blockIdx.x / a.wg_per_pair, e0 = (blockIdx.x % a.wg_per_pair) * RE;
    const int64_t out = (int64_t)pair * a.E;
    const MlgCrossplayPair pr = a.pairs[pair];
    const int U = sh.U, N = sh.N, A = sh.A, nh = sh.nh;
    // As crossplay_kernel: a device pair row that is out of range plays nothing (ep_len -1) instead of reading past
    // the pool or the spec array.
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
            floatx4 x[HC];
            ff_hidden<H, false>(Wv, L, in, x, lane);
            const int32_t* av = valid ? R.lavail + (e * N + ag) * A : nullptr;
            ArgmaxState as{-INFINITY, 1 << 30};
            for (int at = 0; at < n_at; ++at) {
                const floatx4 q = agent_q_tile<H>(Wv, x, at, lane);
                argmax_accumulate(as, q, av, at, A, lane);
            }
            const int act = argmax_reduce(as);
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

// One thread per packed float of one row (blockIdx.y = the row); pack_ff_kernel's arithmetic (pack_ff_elem).
__global__ void pack_ff_pool_kernel(AgentLayout L, const float* __restrict__ flat, int64_t row_stride,
                                    float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.total) return;
    const float* f = flat + (int64_t)blockIdx.y * row_stride;
    const int64_t H = L.H;
    MlgFFParams p;  // DQNAgentNetwork.PARAM_ORDER
    p.fc1_w = f;
    p.fc1_b = p.fc1_w + H * L.d_in;
    p.fc2_w = p.fc1_b + H;
    p.fc2_b = p.fc2_w + (int64_t)L.A * H;
    out[(int64_t)blockIdx.y * L.total + i] = pack_ff_elem(L, p, i);
}

template <int H, int TPW>
int launch_crossplay_ff(const CpLaunch& cl, hipStream_t s, const AgentLayout& L) {
    const size_t bytes = (size_t)cl.lay.total * 4;
    auto kern = crossplay_ff_kernel<H, TPW>;
    if (int rc = allow_lds(kern, bytes, "crossplay_ff")) return rc;
    hipLaunchKernelGGL(kern, dim3(cl.grid), dim3(cl.threads), bytes, s, cl.a, cl.sh, L, cl.lay);
    return 0;
}

}  // namespace

// The rows kept per step do not depend on the agent: mlg_crossplay_workspace_floats' figure under this entry's name.
extern "C" int64_t mlg_crossplay_ff_workspace_floats(const MlgAgentDims* dims, int32_t n_pairs, int32_t E) {
    return cp_workspace_floats(dims, n_pairs, E);
}

extern "C" int mlg_crossplay_rollout_ff(const MlgAgentDims* dims, const MlgCrossplay* c, void* stream) {
    if (check_crossplay_dims(dims)) return 1;
    const AgentLayout L = make_ff_layout(*dims);
    CpLaunch cl;
    if (int rc = cp_prepare(dims, c, L, 0, 0, false, &cl)) return rc;
    hipStream_t s = (hipStream_t)stream;
    int rc = 0;
#define MLG_CP_H(HH)                                                \
    do {                                                            \
        if (cl.tpw == 1) rc = launch_crossplay_ff<HH, 1>(cl, s, L); \
        else if (cl.tpw == 2) rc = launch_crossplay_ff<HH, 2>(cl, s, L); \
        else if (cl.tpw == 3) rc = launch_crossplay_ff<HH, 3>(cl, s, L); \
        else rc = launch_crossplay_ff<HH, 4>(cl, s, L);             \
    } while (0)
    if (L.H == 64) MLG_CP_H(64);
    else if (L.H == 32) MLG_CP_H(32);
    else if (L.H == 128) MLG_CP_H(128);
    else return mlg::fail("crossplay_ff: rnn_hidden_dim=%d unsupported (32, 64, 128)", L.H);
#undef MLG_CP_H
    if (rc) return rc;
    if (mlg::check_launch("crossplay_ff_kernel")) return 1;
    return cp_launch_summary(c, s);
}

extern "C" int mlg_ff_pack_pool(const MlgAgentDims* dims, const float* flat, int64_t row_stride, int32_t P,
                                float* packed_pool, void* stream) {
    if (check_agent_dims(dims)) return 1;
    MLG_REQUIRE(flat && packed_pool, "ff_pack_pool: null pointer");
    MLG_REQUIRE(P >= 1 && P <= 65535, "ff_pack_pool: P=%d must be in [1, 65535]", P);
    const AgentLayout L = make_ff_layout(*dims);
    const int64_t H = L.H;
    const int64_t n_params = H * L.d_in + H + (int64_t)L.A * H + L.A;
    MLG_REQUIRE(row_stride >= n_params, "ff_pack_pool: row_stride=%lld < %lld parameters of the agent",
                (long long)row_stride, (long long)n_params);
    hipLaunchKernelGGL(pack_ff_pool_kernel, dim3((unsigned)((L.total + 255) / 256), (unsigned)P), dim3(256), 0,
                       (hipStream_t)stream, L, flat, row_stride, packed_pool);
    return mlg::check_launch("pack_ff_pool_kernel");
}
