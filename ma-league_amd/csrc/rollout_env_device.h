// rollout_env_device.h -- the per-workgroup env machinery of the fused rollouts, once: spec tables in LDS, the env
// LDS carve, policy sides, observation / reset / env step / full-write zeroing / run summary, action recording and
// the generic kernel's LDS layout. Included by rollout.hip (every ParallelStepper / self-play kernel),
// rollout_policy.hip (COMA's multinomial rollout) and crossplay.hip (league evaluation); file-local in each.
//
// The phase functions take the caller's stamp hooks as a template parameter (anything with mark(int)): rollout.hip
// passes its Stamps (cycle counters in the -DMLG_STAMPS diagnostic build, RoNoStamps otherwise), rollout_policy.hip
// RoNoStamps.
#pragma once
#include "agent_device.h"

namespace {

constexpr int RE = 16;  // envs per workgroup

struct RoNoStamps {  // the rollout's diagnostic phase stamps, compiled out
    __device__ void init() {}
    __device__ void mark(int) {}
    __device__ void step(int, int) {}
    __device__ void flush() {}
};

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

// ---- per-workgroup env bookkeeping shared by the rollout kernels ---------------------------------
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
template <class SP>
__device__ void ro_observe(const EnvTables& T, const MlgEnvSpec& spec, const RoEnv& R, const Sides& sd, int t,
                           bool stepped_only, float inv_p, SP& sp) {
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
// SP: the caller's stamp type; the reset's own phases go to a throw-away instance.
template <class SP>
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
    SP none;
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
template <class SP>
__device__ void ro_env_step(const EnvTables& T, const SpecShared& SS, const MlgEnvSpec& spec, const RoEnv& R,
                            const Sides& sd, const MlgRunInfo& info, int e0, int t, float inv_p, SP& sp) {
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

// Dynamic-LDS layout of the generic kernels (rollout_kernel, rollout_policy_kernel): the packed weights when they
// fit, then the env part.
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

}  // namespace
