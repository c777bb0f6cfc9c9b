// rollout_policy.hip -- one ParallelStepper.run with a pi_logits MAC (COMA): mlg_rollout_policy.
//
// The generic fp32 rollout kernel (rollout.hip's rollout_kernel: a workgroup owns RE = 16 envs for the whole episode,
// wave w owns the 16-row agent tiles w, w + W, ..., GRU hidden state in VGPRs, env state in LDS) with the selection
// site replaced: instead of the masked argmax + epsilon-greedy pick, the agent's outputs go through the policy softmax
// with the epsilon floor (MultiAgentController._softmax, multi_agent_controller.py:78-99) and the action is drawn by
// the multinomial rule of mlg_select_multinomial (MultinomialActionSelector.select, action_selectors.py:11-32) on the
// counter RNG, or is the first-index argmax with test_mode and test_greedy. Env step, observation, reset, ring /
// full-write modes and the run summary are the generic kernel's, bit for bit.
//
// The env-side device code (SpecShared .. ro_record_action, RolloutLds) restates rollout.hip's, file-local there. It
// is repeated here, not moved to a shared header, because rollout.hip is pinned: the committed one-env step stamp
// behind the bench's latency floor (profiles/counters.json, tests/test_bench_counters.py) is tied to that file's last
// commit (crossplay.hip does the same).
#include <cstdlib>
#include <cstring>

#include "agent_device.h"
#include "coma_device.h"
#include "mlg_host.h"

int check_agent_dims(const MlgAgentDims* d);  // agent.hip

namespace {

struct Stamps {  // the phase stamps of the diagnostic build belong to rollout.hip's kernels
    __device__ void init() {}
    __device__ void mark(int) {}
    __device__ void step(int, int) {}
    __device__ void flush() {}
};

constexpr int RE = 16;  // envs per workgroup

struct SpecShared {
    int team[MLG_MAXU], role[MLG_MAXU], melee[MLG_MAXU], agent[MLG_MAXU];
    int aunit[MLG_MAXU];  // unit of agent a
    int team_first[2], team_size[2];
};

__device__ void load_spec_tables(const MlgEnvSpec& spec, SpecShared& s) {
    const int tid = threadIdx.x;
    for (int u = tid; u < MLG_MAXU; u += blockDim.x) {
        const bool in = u < spec.U;
        s.team[u] = in ? spec.team[u] : 0;
        s.role[u] = in ? spec.role[u] : 0;
        s.melee[u] = in ? spec.melee[u] : 0;
        s.agent[u] = 0;
    }
    __syncthreads();
    for (int a = tid; a < spec.n_agents; a += blockDim.x) {
        s.agent[spec.agent_unit[a]] = a + 1;
        s.aunit[a] = spec.agent_unit[a];
    }
    if (tid == 0) {
        for (int tm = 0; tm < 2; ++tm) {
            s.team_first[tm] = -1;
            s.team_size[tm] = 0;
        }
        for (int u = 0; u < spec.U; ++u) {
            const int tm = spec.team[u];
            if (s.team_first[tm] < 0) s.team_first[tm] = u;
            s.team_size[tm]++;
        }
    }
    __syncthreads();
}

__device__ __forceinline__ EnvTables make_tables(const MlgEnvSpec& spec, const SpecShared& s) {
    EnvTables T;
    T.team = s.team;
    T.role = s.role;
    T.melee = s.melee;
    T.agent = s.agent;
    T.U = spec.U;
    T.grid = spec.grid;
    T.episode_limit = spec.episode_limit;
    T.stochastic = spec.stochastic;
    return T;
}

// ---- per-workgroup env bookkeeping shared by both rollout kernels --------------------------------
// LDS pointers of the RE envs a workgroup owns. lobs/lavail (v2 only, else nullptr) mirror the obs and
// avail rows the agent phase reads, so the cell never reads back what the env phase wrote to HBM.
struct RoEnv {
    int *x, *y, *hp, *nhp, *act, *pact, *prev, *status, *stepped, *len, *slot, *list, *misc;
    int* slot2;  // batch slot of the away side (self-play, v1 only)
    uint32_t* episode;
    float *ret, *ret2;  // episode return of side 0 (home / policy team) and side 1 (away)
    float* lobs;
    int32_t* lavail;
    int ldo;
};

// Dynamic-LDS carve of the env part (4-byte words).
struct RoEnvLds {
    int32_t spec, x, y, hp, nhp, act, pact, prev, status, stepped, len, episode, ret, slot, list, misc, slot2, ret2;
};

__host__ __device__ constexpr int64_t ro_take(int64_t& o, int64_t n) {
    const int64_t v = o;
    o += mlg_align4(n);
    return v;
}

// The fields the v2-structure env lanes use (status, episode, slot, pending / previous actions); the others alias
// offset 0 and are never dereferenced by those kernels.
__host__ __device__ constexpr RoEnvLds make_env_lds_v2(int64_t& o, int n_agents, int re) {
    RoEnvLds r{};
    r.spec = ro_take(o, (int64_t)(sizeof(SpecShared) / 4));
    r.pact = ro_take(o, (int64_t)re * n_agents);
    r.prev = ro_take(o, (int64_t)re * n_agents);
    r.status = ro_take(o, re);
    r.episode = ro_take(o, re);
    r.slot = ro_take(o, re);
    return r;
}

__host__ __device__ constexpr RoEnvLds make_env_lds(int64_t& o, int U, int n_agents, int re = RE) {
    RoEnvLds r{};
    r.spec = ro_take(o, (int64_t)(sizeof(SpecShared) / 4));
    const int64_t eu = (int64_t)re * U;
    r.x = ro_take(o, eu);
    r.y = ro_take(o, eu);
    r.hp = ro_take(o, eu);
    r.nhp = ro_take(o, eu);
    r.act = ro_take(o, eu);
    r.pact = ro_take(o, (int64_t)re * n_agents);
    r.prev = ro_take(o, (int64_t)re * n_agents);
    r.status = ro_take(o, re);
    r.stepped = ro_take(o, re);
    r.len = ro_take(o, re);
    r.episode = ro_take(o, re);
    r.ret = ro_take(o, re);
    r.slot = ro_take(o, re);
    r.list = ro_take(o, re);
    r.misc = ro_take(o, 4);  // [0] any env running, [1] number of running envs
    r.slot2 = ro_take(o, re);
    r.ret2 = ro_take(o, re);
    return r;
}

__device__ inline RoEnv env_view(int* smem, const RoEnvLds& l) {
    RoEnv R;
    R.x = smem + l.x;
    R.y = smem + l.y;
    R.hp = smem + l.hp;
    R.nhp = smem + l.nhp;
    R.act = smem + l.act;
    R.pact = smem + l.pact;
    R.prev = smem + l.prev;
    R.status = smem + l.status;
    R.stepped = smem + l.stepped;
    R.len = smem + l.len;
    R.slot = smem + l.slot;
    R.list = smem + l.list;
    R.misc = smem + l.misc;
    R.episode = reinterpret_cast<uint32_t*>(smem + l.episode);
    R.ret = reinterpret_cast<float*>(smem + l.ret);
    R.slot2 = smem + l.slot2;
    R.ret2 = reinterpret_cast<float*>(smem + l.ret2);
    R.lobs = nullptr;
    R.lavail = nullptr;
    R.ldo = 0;
    return R;
}

// Policy sides of a rollout. ns = 1: one MAC acts for the policy team (ParallelStepper). ns = 2: self-play
// (self_play_parallel_stepper.py:97-108): agents [0, nh) are the home team and act with P[0] into bt[0],
// agents [nh, 2 nh) the away team with P[1] into bt[1]; stepper_utils.build_pre_transition_data
// (stepper_utils.py:4-24) splits obs / avail the same way, state goes to both batches.
struct Sides {
    MlgBatch bt[2];
    const float* P[2];
    float eps[2];
    int ns, nh;
};

// Field selects instead of dynamic indexing: keeps the kernel-argument struct in SGPRs (no scratch copy).
__device__ __forceinline__ MlgBatch side_batch(const Sides& sd, int side) { return side ? sd.bt[1] : sd.bt[0]; }
__device__ __forceinline__ int side_slot(const RoEnv& R, int side, int e) { return side ? R.slot2[e] : R.slot[e]; }

// obs/state/avail of batch time index t for the envs selected by `sel` (0: not done at reset, 1: stepped).
__device__ void ro_observe(const EnvTables& T, const MlgEnvSpec& spec, const RoEnv& R, const Sides& sd, int t,
                           bool stepped_only, float inv_p, Stamps& sp) {
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int U = T.U, N = spec.n_agents, A = spec.n_actions, S = 6 * U, DO = 8 * U, T1 = sd.bt[0].T1, nh = sd.nh;
    auto on = [&](int e) { return stepped_only ? R.stepped[e] != 0 : R.status[e] != 2; };
    for (int i = tid; i < RE * N * U; i += nthr) {
        const int e = i / (N * U), r = i % (N * U);
        if (!on(e)) continue;
        const int a = r / U, j = r % U;
        const int side = a >= nh, ln = a - side * nh;
        float o[8];
        env_obs_feat(T, R.x + e * U, R.y + e * U, R.hp + e * U, spec.agent_unit[a], j, inv_p, o);
        const floatx4 lo{o[0], o[1], o[2], o[3]}, hi{o[4], o[5], o[6], o[7]};
        float* dst = side_batch(sd, side).obs + (((int64_t)side_slot(R, side, e) * T1 + t) * nh + ln) * DO + j * 8;
        *reinterpret_cast<floatx4*>(dst) = lo;
        *reinterpret_cast<floatx4*>(dst + 4) = hi;
        if (R.lobs) {
            float* l = R.lobs + (e * N + a) * R.ldo + j * 8;
            *reinterpret_cast<floatx4*>(l) = lo;
            *reinterpret_cast<floatx4*>(l + 4) = hi;
        }
    }
    sp.mark(7);
    for (int i = tid; i < RE * U; i += nthr) {
        const int e = i / U, j = i % U;
        if (!on(e)) continue;
        float o[6];
        env_state_feat(T, R.x + e * U, R.y + e * U, R.hp + e * U, j, inv_p, o);
        for (int side = 0; side < sd.ns; ++side) {
            float* dst = side_batch(sd, side).state + ((int64_t)side_slot(R, side, e) * T1 + t) * S + j * 6;
#pragma unroll
            for (int f = 0; f < 6; ++f) dst[f] = o[f];
        }
    }
    sp.mark(8);
    for (int i = tid; i < RE * N * A; i += nthr) {
        const int e = i / (N * A), r = i % (N * A);
        if (!on(e)) continue;
        const int a = r / A, side = a >= nh;
        const int v = env_avail_one(T, R.x + e * U, R.y + e * U, R.hp + e * U, spec.agent_unit[a], r % A);
        side_batch(sd, side).avail[((int64_t)side_slot(R, side, e) * T1 + t) * nh * A + r - side * nh * A] = v;
        if (R.lavail) R.lavail[e * N * A + r] = v;
    }
    sp.mark(9);
}

__device__ __forceinline__ int ring_slot_of(const MlgBatch& b, int env) {
    return b.ring_size > 0 ? (b.ring_slot0 + env) % b.ring_size : env;
}

// Reset of the RE envs (parallel_stepper.py:82-104; env_worker_process.py:54-60) + observation at t = 0.
__device__ void ro_reset(const EnvTables& T, const SpecShared& SS, const MlgEnvSpec& spec, const MlgEnvState& st,
                         const RoEnv& R, const Sides& sd, int e0, float inv_p) {
    const int tid = threadIdx.x, nthr = blockDim.x, U = T.U, B = sd.bt[0].B;
    for (int e = tid; e < RE; e += nthr) {
        const int b = e0 + e;
        R.len[e] = 0;
        R.ret[e] = 0.f;
        R.ret2[e] = 0.f;
        R.stepped[e] = 0;
        if (b < B) {
            const uint32_t ep = st.episode[b];
            st.episode[b] = ep + 1;
            R.episode[e] = ep;
            R.status[e] = 0;
            R.slot[e] = ring_slot_of(sd.bt[0], b);
            R.slot2[e] = ring_slot_of(sd.bt[1], b);
            for (int side = 0; side < sd.ns; ++side) {
                const MlgBatch bt = side_batch(sd, side);
                bt.filled[(int64_t)side_slot(R, side, e) * bt.T1] = 1;
            }
        } else {
            R.status[e] = 2;
        }
    }
    __syncthreads();
    for (int i = tid; i < RE * U; i += nthr) {
        const int e = i / U, u = i % U;
        if (R.status[e] == 2) continue;
        const int tm = SS.team[u];
        env_spawn_unit(T, mlg_env_key(spec.seed, e0 + e), R.episode[e], u, SS.team_first[tm], SS.team_size[tm],
                       R.x + e * U, R.y + e * U, R.hp + e * U);
    }
    __syncthreads();
    Stamps none;
    ro_observe(T, spec, R, sd, 0, false, inv_p, none);
}

// Running-env list (status < 2, ascending) and count; single thread, caller syncs.
__device__ inline void ro_list_running(const RoEnv& R) {
    int n = 0;
    for (int e = 0; e < RE; ++e)
        if (R.status[e] < 2) R.list[n++] = e;
    R.misc[0] = n > 0;
    R.misc[1] = n;
}

// Env phase of step t for the running envs (env_worker_process.py:32-53 batched): executed actions
// (policy or scripted AI), simultaneous resolution, per-env reward / termination, then obs of t + 1.
// Side s receives the reward of its own team (self-play: reward = (home, away), self_play_parallel_stepper.py:159).
__device__ void ro_env_step(const EnvTables& T, const SpecShared& SS, const MlgEnvSpec& spec, const RoEnv& R,
                            const Sides& sd, const MlgRunInfo& info, int e0, int t, float inv_p, Stamps& sp) {
    const int tid = threadIdx.x, nthr = blockDim.x, U = T.U, N = spec.n_agents, T1 = sd.bt[0].T1;
    for (int i = tid; i < RE * U; i += nthr) {
        const int e = i / U, u = i % U;
        if (R.status[e] != 0) continue;
        const int ag = SS.agent[u];
        R.act[e * U + u] = env_exec_action(T, R.x + e * U, R.y + e * U, R.hp + e * U, u,
                                           ag ? (int64_t)R.pact[e * N + ag - 1] : 0);
    }
    sp.mark(4);
    __syncthreads();
    for (int i = tid; i < RE * U; i += nthr) {
        const int e = i / U, j = i % U;
        if (R.status[e] != 0) continue;
        R.nhp[e * U + j] = env_resolve_hp(T, R.act + e * U, R.hp + e * U, j);
        if (R.hp[e * U + j] > 0) env_apply_move(R.act[e * U + j], &R.x[e * U + j], &R.y[e * U + j]);
    }
    sp.mark(5);
    __syncthreads();
    const int pt = spec.policy_team;  // team of side 0; side 1 (self-play) is the other plan team
    for (int e = tid; e < RE; e += nthr) {
        const int b = e0 + e;
        const int status = R.status[e];
        R.stepped[e] = 0;
        if (status == 2) continue;
        for (int n = 0; n < N; ++n) R.prev[e * N + n] = R.pact[e * N + n];
        if (status == 1) {  // final action recorded; env done (parallel_stepper.py:153)
            R.status[e] = 2;
            for (int side = 0; side < sd.ns; ++side) {
                const MlgBatch bt = side_batch(sd, side);
                if (bt.full_write) {
                    bt.reward[(int64_t)side_slot(R, side, e) * T1 + t] = 0.f;
                    bt.terminated[(int64_t)side_slot(R, side, e) * T1 + t] = 0;
                }
            }
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
        const int done = alive[0] == 0 || alive[1] == 0 || t + 1 >= spec.episode_limit;
        int won[2];
        won[0] = alive[1] == 0 && alive[0] > 0;
        won[1] = alive[0] == 0 && alive[1] > 0;
        for (int side = 0; side < sd.ns; ++side) {
            const int tm = side ? 1 - pt : pt;
            const float r = (float)(lost[1 - tm] + 10 * kills[tm] + 200 * won[tm]) * 0.0625f;
            const MlgBatch bt = side_batch(sd, side);
            const int64_t sl = (int64_t)side_slot(R, side, e) * T1 + t;
            bt.reward[sl] = r;
            bt.terminated[sl] = (uint8_t)done;
            bt.filled[sl + 1] = 1;
            if (side) R.ret2[e] += r;
            else R.ret[e] += r;
        }
        R.stepped[e] = 1;
        if (done) {
            R.status[e] = 1;
            R.len[e] = t + 1;
            info.won[2 * b] = won[pt];
            info.won[2 * b + 1] = won[1 - pt];
            info.draw[b] = !won[0] && !won[1];
        }
    }
    sp.mark(6);
    __syncthreads();
    // observation at t + 1 for envs that stepped (incl. those that just terminated)
    ro_observe(T, spec, R, sd, t + 1, true, inv_p, sp);
}

// Zero every key of slots [t0, t1) of the envs of this workgroup that are done and did not step
// (status 2, or stepped == 0 with status 2 after the final action): the full-write (ring) mode's
// replacement for zero-initialising the EpisodeBatch. Sides in full-write mode only.
__device__ void zero_slots(const Sides& sd, const RoEnv& R, int e0, int t0, int t1, int A, int S, int DO) {
    const int T1 = sd.bt[0].T1, B = sd.bt[0].B, N = sd.nh;
    const int per = S + N * DO + 2 * N * A + 2 * N + 3;  // words per slot (actions/filled are 2 words)
    const int total = sd.ns * RE * (t1 - t0) * per;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int side = i / (RE * (t1 - t0) * per), ii = i % (RE * (t1 - t0) * per);
        const int e = ii / ((t1 - t0) * per), rem = ii % ((t1 - t0) * per);
        const int t = t0 + rem / per;
        int k = rem % per;
        const MlgBatch bt = side_batch(sd, side);
        if (!bt.full_write || e0 + e >= B || R.status[e] != 2 || R.stepped[e]) continue;
        const int64_t sl = (int64_t)side_slot(R, side, e) * T1 + t;
        if (k < S) { bt.state[sl * S + k] = 0.f; continue; }
        k -= S;
        if (k < N * DO) { bt.obs[sl * N * DO + k] = 0.f; continue; }
        k -= N * DO;
        if (k < N * A) { bt.avail[sl * N * A + k] = 0; continue; }
        k -= N * A;
        if (k < N * A) { bt.actions_onehot[sl * N * A + k] = 0.f; continue; }
        k -= N * A;
        if (k < N) { bt.actions[sl * N + k] = 0; continue; }
        k -= N;
        if (k < N) continue;  // (second word of the int64 actions, covered above)
        k -= N;
        if (k == 0) bt.reward[sl] = 0.f;
        else if (k == 1) bt.terminated[sl] = 0;
        else bt.filled[sl] = 0;
    }
}

// Per-env summary + env state write-back.
__device__ void ro_finish(const MlgEnvState& st, const RoEnv& R, const Sides& sd, const MlgRunInfo& info, int e0, int B,
                          int U) {
    const int tid = threadIdx.x, nthr = blockDim.x;
    for (int e = tid; e < RE; e += nthr) {
        const int b = e0 + e;
        if (b >= B) continue;
        info.ep_len[b] = R.len[e];
        info.ret[b] = R.ret[e];
        if (info.ret_away) info.ret_away[b] = R.ret2[e];
        st.t[b] = R.len[e];
        for (int side = 0; side < sd.ns; ++side) {  // v1 zeroes every tail row: the slot's extent is L + 1
            const MlgBatch bt = side_batch(sd, side);
            if (bt.full_write && bt.slot_extent) bt.slot_extent[side_slot(R, side, e)] = R.len[e] + 1;
        }
    }
    for (int i = tid; i < RE * U; i += nthr) {
        const int e = i / U, u = i % U;
        const int64_t b = e0 + e;
        if (b >= B) continue;
        st.x[b * U + u] = R.x[e * U + u];
        st.y[b * U + u] = R.y[e * U + u];
        st.hp[b * U + u] = R.hp[e * U + u];
    }
}

// Picks the action of agent a (global index; side a >= nh) from the masked argmax
// (EpsilonGreedyActionSelector.select, action_selectors.py:44-62) and records it: LDS pending action,
// the side's batch actions / actions_onehot. The epsilon RNG stream index is the global agent index.
__device__ __forceinline__ void ro_record_action(const MlgEnvSpec& spec, const RoEnv& R, const Sides& sd, int act,
                                                 const int32_t* av, int e, int a, int b, int t, int test_mode) {
    const int N = spec.n_agents, A = spec.n_actions, nh = sd.nh;
    const int side = a >= nh, ln = a - side * nh;
    const float eps = side ? sd.eps[1] : sd.eps[0];
    if (!test_mode && eps > 0.f) {
        const uint64_t key = mlg_env_key(spec.seed, b);
        const uint64_t r1 = mlg_rng(key, mlg_ctr(R.episode[e], (uint32_t)t, MLG_PURPOSE_EPS, (uint32_t)a));
        if (mlg_u01(r1) < eps) {
            const uint64_t r2 = mlg_rng(key, mlg_ctr(R.episode[e], (uint32_t)t, MLG_PURPOSE_RAND, (uint32_t)a));
            act = random_available(av, A, r2);
        }
    }
    R.pact[e * N + a] = act;
    const MlgBatch bt = side_batch(sd, side);
    const int64_t bt_off = ((int64_t)side_slot(R, side, e) * bt.T1 + t) * nh + ln;
    bt.actions[bt_off] = act;
    if (bt.full_write)
        for (int k = 0; k < A; ++k) bt.actions_onehot[bt_off * A + k] = k == act ? 1.0f : 0.0f;
    else
        bt.actions_onehot[bt_off * A + act] = 1.0f;
}

// ================================================================================================
// v1: generic kernel (any H in {32, 64, 128}, weights in LDS or HBM; the only kernel with self-play sides).
// Workgroup = W waves (W = min(tiles, 8)); wave w owns the 16-row agent tiles w, w + W, ... for the whole
// episode with the GRU hidden state in VGPRs. Tiles never mix sides: side s owns tiles [s tps, (s+1) tps),
// row r of side s = env (r / nh), agent s nh + r % nh.
struct RolloutLds {
    int32_t wts, total;
    RoEnvLds env;
    LdsWeights lw;
    int weights_in_lds;
};

__host__ __device__ inline RolloutLds make_rollout_lds(const AgentLayout& L, int U, int n_agents, bool weights_in_lds) {
    RolloutLds r;
    r.lw = make_lds_weights(L);
    r.weights_in_lds = weights_in_lds;
    int64_t o = 0;
    r.wts = ro_take(o, weights_in_lds ? r.lw.total : 0);
    r.env = make_env_lds(o, U, n_agents);
    r.total = o;
    return r;
}

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
    ro_reset(T, SS, spec, st, R, sd, e0, inv_p);
    __syncthreads();

    floatx4 h[TPW][HC];
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
        for (int c = 0; c < HC; ++c) h[ti][c] = floatx4{0.f, 0.f, 0.f, 0.f};
    Stamps sp;
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


int check_spec(const MlgEnvSpec* s) {
    MLG_REQUIRE(s != nullptr, "null spec");
    MLG_REQUIRE(s->U >= 2 && s->U <= MLG_MAXU, "spec.U=%d out of range [2, %d]", s->U, MLG_MAXU);
    MLG_REQUIRE(s->n_agents >= 1 && s->n_agents <= s->U, "spec.n_agents=%d invalid", s->n_agents);
    MLG_REQUIRE(s->n_actions == MLG_ACT_BASE + s->U, "spec.n_actions must be 5+U");
    MLG_REQUIRE(s->grid >= 2 && s->grid <= 4096, "spec.grid=%d invalid", s->grid);
    MLG_REQUIRE(s->episode_limit >= 1 && s->episode_limit < 65535, "spec.episode_limit invalid");
    MLG_REQUIRE(s->policy_team == 0 || s->policy_team == 1, "spec.policy_team invalid");
    for (int u = 0; u < s->U; ++u) {
        MLG_REQUIRE(s->team[u] == 0 || s->team[u] == 1, "unit %d team invalid", u);
        MLG_REQUIRE(s->role[u] >= 0 && s->role[u] <= 2, "unit %d role invalid", u);
        MLG_REQUIRE(s->melee[u] == 0 || s->melee[u] == 1, "unit %d attack type invalid", u);
    }
    for (int a = 0; a < s->n_agents; ++a)
        MLG_REQUIRE(s->agent_unit[a] >= 0 && s->agent_unit[a] < s->U, "agent %d unit invalid", a);
    return 0;
}

int check_state(const MlgEnvState* st) {
    MLG_REQUIRE(st && st->x && st->y && st->hp && st->t && st->episode, "env state has null pointers");
    MLG_REQUIRE(st->B >= 1, "env state B=%d", st->B);
    return 0;
}


int check_rollout_batch(const MlgBatch* batch, const MlgEnvSpec* spec, const MlgEnvState* st, const char* who) {
    MLG_REQUIRE(batch, "%s: null batch", who);
    MLG_REQUIRE(batch->state && batch->obs && batch->actions && batch->avail && batch->reward && batch->terminated &&
                    batch->actions_onehot && batch->filled,
                "%s: batch has null tensors", who);
    MLG_REQUIRE(batch->B == st->B, "%s: batch B=%d != env B=%d", who, batch->B, st->B);
    MLG_REQUIRE(batch->rows == nullptr, "%s: sampled (rows) views are read-only; use ring mode to write slots", who);
    MLG_REQUIRE(batch->T1 == spec->episode_limit + 1, "%s: batch T1=%d != episode_limit+1=%d", who, batch->T1,
                spec->episode_limit + 1);
    MLG_REQUIRE(batch->ring_size == 0 || (batch->ring_size >= batch->B && batch->ring_slot0 >= 0 &&
                                          batch->ring_slot0 < batch->ring_size),
                "%s: bad ring (slot0=%d size=%d B=%d)", who, batch->ring_slot0, batch->ring_size, batch->B);
    return 0;
}

constexpr int LDS_LIMIT_BYTES = 160 * 1024;

template <int H, int TPW, bool WLDS>
int launch_policy_t(int grid, int threads, hipStream_t s, const MlgEnvSpec& spec, const MlgEnvState& st,
                    const AgentLayout& L, const Sides& sd, const MlgRunInfo& info, int flags, const RolloutLds& lay) {
    const size_t bytes = (size_t)lay.total * 4;
    auto kern = rollout_policy_kernel<H, TPW, WLDS>;
    if (bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)bytes);
        if (e != hipSuccess) return mlg::fail("rollout_policy: LDS attribute (%zu B): %s", bytes, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), bytes, s, spec, st, L, sd, info, flags, lay);
    return 0;
}

// Weights in LDS when the policy's image fits next to the env state, else read from HBM / L2.
template <int H, int TPW>
int launch_policy(int grid, int threads, hipStream_t s, const MlgEnvSpec& spec, const MlgEnvState& st,
                  const AgentLayout& L, const Sides& sd, const MlgRunInfo& info, int flags) {
    RolloutLds lay = make_rollout_lds(L, spec.U, spec.n_agents, true);
    if (lay.total * 4 <= LDS_LIMIT_BYTES)
        return launch_policy_t<H, TPW, true>(grid, threads, s, spec, st, L, sd, info, flags, lay);
    lay = make_rollout_lds(L, spec.U, spec.n_agents, false);
    MLG_REQUIRE(lay.total * 4 <= LDS_LIMIT_BYTES, "rollout_policy: the env state of %d units does not fit in LDS", spec.U);
    return launch_policy_t<H, TPW, false>(grid, threads, s, spec, st, L, sd, info, flags, lay);
}

}  // namespace

extern "C" int mlg_rollout_policy(const MlgEnvSpec* spec, MlgEnvState* st, const MlgAgentDims* dims,
                                  const float* packed, MlgBatch* batch, MlgRunInfo* info, float epsilon,
                                  int32_t test_mode, int32_t mask_before_softmax, int32_t test_greedy, void* stream) {
    if (check_spec(spec) || check_state(st) || check_agent_dims(dims)) return 1;
    MLG_REQUIRE(packed && batch && info, "rollout_policy: null pointer");
    if (check_rollout_batch(batch, spec, st, "rollout_policy")) return 1;
    MLG_REQUIRE(info->ep_len && info->ret && info->won && info->draw, "rollout_policy: run info has null tensors");
    MLG_REQUIRE(dims->n_agents == spec->n_agents && dims->n_actions == spec->n_actions && dims->d_obs == 8 * spec->U,
                "rollout_policy: agent dims do not match env spec (N=%d/%d A=%d/%d d_obs=%d/%d)", dims->n_agents,
                spec->n_agents, dims->n_actions, spec->n_actions, dims->d_obs, 8 * spec->U);
    const AgentLayout L = make_agent_layout(*dims);
    MLG_REQUIRE(L.Ap <= 16 * RO_MAXAT, "rollout_policy: n_actions=%d does not fit %d action tiles", dims->n_actions,
                RO_MAXAT);
    hipStream_t s = (hipStream_t)stream;
    Sides sd;
    sd.bt[0] = sd.bt[1] = *batch;
    sd.P[0] = sd.P[1] = packed;
    sd.eps[0] = sd.eps[1] = test_mode ? 0.f : epsilon;
    sd.ns = 1;
    sd.nh = spec->n_agents;
    const int flags = (test_mode ? 1 : 0) | (mask_before_softmax ? 2 : 0) | (test_greedy ? 4 : 0);
    const int tiles = (RE * sd.nh + 15) / 16;
    const int W = tiles < 8 ? tiles : 8;
    const int tpw = (tiles + W - 1) / W;
    const int grid = (st->B + RE - 1) / RE;
    const int threads = W * 64;
    int rc = 0;
    MLG_REQUIRE(tpw <= 4, "rollout_policy: %d agent tiles per wave > 4 (too many agents per env)", tpw);
#define MLG_RO(HH, TT) rc = launch_policy<HH, TT>(grid, threads, s, *spec, *st, L, sd, *info, flags)
#define MLG_RO_H(HH)          \
    if (tpw == 1) MLG_RO(HH, 1);      \
    else if (tpw == 2) MLG_RO(HH, 2); \
    else if (tpw == 3) MLG_RO(HH, 3); \
    else MLG_RO(HH, 4)
    if (L.H == 64) {
        MLG_RO_H(64);
    } else if (L.H == 32) {
        MLG_RO_H(32);
    } else if (L.H == 128) {
        MLG_RO_H(128);
    } else {
        return mlg::fail("rollout_policy: rnn_hidden_dim=%d unsupported (32, 64, 128)", L.H);
    }
#undef MLG_RO_H
#undef MLG_RO
    if (rc) return rc;
    return mlg::check_launch("rollout_policy_kernel");
}
