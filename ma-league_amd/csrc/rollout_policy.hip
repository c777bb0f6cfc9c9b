// rollout_policy.hip -- one ParallelStepper.run with a pi_logits MAC (COMA): mlg_rollout_policy.
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

// Multinomial policy pick for the lane's row (mlg_rollout_policy: MultiAgentController._softmax,
// multi_agent_controller.py:78-99, then MultinomialActionSelector.select, action_selectors.py:11-32, with the draw rule
// of mlg_select_multinomial). qt[at][r] is the logit of action 16 at + 4 g + r; the four lanes col + 16 g of a row
// share the work and every one returns the action. Sums add each lane's four entries first, then the lanes in
// ascending g, then the tiles in ascending order. All 64 lanes must be active; av == nullptr: every action available.
constexpr int RO_MAXAT = 5;  // n_actions = 5 + U <= 69 fits five 16-wide tiles
__device__ __forceinline__ int ro_policy_select(floatx4 (&qt)[RO_MAXAT], int n_at, const int32_t* av, int A, int lane,
                                                float eps, bool mask, bool test_mode, bool greedy, float u) {
    const int g = lane >> 4;
    auto xor_f = [](float v, int m) { return __shfl_xor(v, m); };
    unsigned ok = 0u;  // bit 4 at + r: the action is in range and available
    float mx = -INFINITY;
#pragma unroll
    for (int at = 0; at < RO_MAXAT; ++at)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int a = at * 16 + 4 * g + r;
            const bool in = at < n_at && a < A;
            const bool on = in && (av == nullptr || av[a] != 0);
            ok |= (unsigned)on << (4 * at + r);
            const float x = in ? ((mask && !on) ? -1e10f : qt[at][r]) : -INFINITY;
            qt[at][r] = x;
            mx = fmaxf(mx, x);
        }
    mx = fmaxf(mx, xor_f(mx, 16));
    mx = fmaxf(mx, xor_f(mx, 32));
    int K = __popc(ok);
    K += __shfl_xor(K, 16);
    K += __shfl_xor(K, 32);
    float s = 0.f;
#pragma unroll
    for (int at = 0; at < RO_MAXAT; ++at)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            qt[at][r] = expf(qt[at][r] - mx);  // exp(-inf) = 0 for the entries out of range
            s += qt[at][r];
        }
    s += xor_f(s, 16);
    s += xor_f(s, 32);
    const float keep = 1.f - eps, floor_p = eps / (float)(mask ? K : A);
    // m_k: the probability where available, else 0
#pragma unroll
    for (int at = 0; at < RO_MAXAT; ++at)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = qt[at][r] / s;
            qt[at][r] = ((ok >> (4 * at + r)) & 1u) ? (test_mode ? p : keep * p + floor_p) : 0.f;
        }
    if (greedy) {
        ArgmaxState as{-INFINITY, 1 << 30};
#pragma unroll
        for (int at = 0; at < RO_MAXAT; ++at)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a = at * 16 + 4 * g + r;
                const float v = ((ok >> (4 * at + r)) & 1u) ? qt[at][r] : -INFINITY;
                if (a < A && amax_better(v, a, as.bv, as.bi)) { as.bv = v; as.bi = a; }
            }
        const int act = argmax_reduce(as);
        return act < A ? act : 0;
    }
    const int col = lane & 15;
    float total = 0.f;
#pragma unroll
    for (int at = 0; at < RO_MAXAT; ++at) {
        const float ls = ((qt[at][0] + qt[at][1]) + qt[at][2]) + qt[at][3];
        total = (((total + __shfl(ls, col)) + __shfl(ls, col + 16)) + __shfl(ls, col + 32)) + __shfl(ls, col + 48);
    }
    const float thr = u * total;
    float run = 0.f;
    int pick = 1 << 30, last = -1;
#pragma unroll
    for (int at = 0; at < RO_MAXAT; ++at) {
        const float ls = ((qt[at][0] + qt[at][1]) + qt[at][2]) + qt[at][3];
        const float s0 = __shfl(ls, col), s1 = __shfl(ls, col + 16), s2 = __shfl(ls, col + 32),
                    s3 = __shfl(ls, col + 48);
        float c = run;
        if (g > 0) c += s0;
        if (g > 1) c += s1;
        if (g > 2) c += s2;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (!((ok >> (4 * at + r)) & 1u)) continue;
            const int a = at * 16 + 4 * g + r;
            c += qt[at][r];
            last = a;
            if (pick == (1 << 30) && c > thr) pick = a;
        }
        run = (((run + s0) + s1) + s2) + s3;
    }
    pick = min(pick, __shfl_xor(pick, 16));
    pick = min(pick, __shfl_xor(pick, 32));
    last = max(last, __shfl_xor(last, 16));
    last = max(last, __shfl_xor(last, 32));
    return pick != (1 << 30) ? pick : (last >= 0 ? last : 0);
}

// flags: bit 0 test_mode, bit 1 mask_before_softmax, bit 2 test_greedy. One policy side (sd.ns = 1).
// The body is rollout_kernel's (rollout.hip) line for line but for the selection site; it is written out twice because
// a shared __forceinline__ body with the selection passed in as a callable made the compiler allocate registers
// differently in every instantiation of both kernels.
template <int H, int TPW, bool WLDS>
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
            const WView Wv = WLDS ? lds_view(reinterpret_cast<const float*>(smem + lay.wts) + zero, lay.lw, L)
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
            const int act = ro_policy_select(qt, n_at, av, A, lane, sd.eps[0], (flags & 2) != 0, tm, greedy, u);
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
