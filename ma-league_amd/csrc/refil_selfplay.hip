// refil_selfplay.hip -- REFIL in self-play (DESIGN.md §3b', §4c''): two EntityMACs play each other over the two-policy
// entity env in one launch.
//
//   mlg_refil_rollout_selfplay           SelfPlayParallelStepper.run over the entity env, an EntityMAC on each side
//   mlg_refil_rollout_selfplay_describe  the arm that launch takes (host only)
//
// Structure of refil.hip's two-env kernel (refil_rollout_kernel<KC1>): one wave owns two envs for the whole episode,
// env lanes 0..31 step the env with the unit state in the wave's LDS, the agent phase builds the entity block per env
// and runs both envs' 2 x 8 agent rows as one 16-row tile. Here the agent phase runs once per side with that side's
// weights, hidden state, view and pending actions; the env phase has no scripted-AI branch.
//
// Views. Home (side 0) sees the raw state: entities in unit order, raw action indices. Away (side 1) sees the canonical
// view of §3b': entity j' is unit (j' + S) mod U (its own team first), x mirrored (G - 1 - x), team flipped, move
// actions 3 / 4 swapped, target 5 + j' = raw target 5 + (j' + S) mod U. With U = 2S that index map is "swap the two
// halves": on a U-bit mask it is a rotation by S bits (view_rot). Everything the away side reads or records (entity
// rows, mask rows, avail, actions, one-hot rows, last-action columns) is in canonical indices; the env executes the raw
// image of the chosen action.
#include <cstring>

#include "mlg_host.h"
#include "refil_device.h"
#include "refil_host.h"
#include "refil_rollout_device.h"

using namespace refil;

namespace {

struct SpLds {
    float q[NAS * LDX];
    float kv[NE * LDKV];
    float o[16 * LDX];
    float feat[2][2][NE][8];  // [side][env][entity of the side's view]
    uint32_t om[2][2][NE];    // [side][env][row entity of the side's view], bits in view order
    uint32_t em[2][2];        // [side][env]
    uint32_t av[2][2][NAS];   // [side][env][agent], action bits in view indices
    alignas(16) int pk[2][NE];  // packed unit states x | y << 8 | hp << 16 (register env rules)
    alignas(16) int act[2][NE];
    int x[2][NE], y[2][NE], hp[2][NE], nhp[2][NE];
    int pact[2][2][NAS];  // [side][env][agent] pending action, view index
    int team[NE], role[NE], melee[NE], agent[NE];
    int status[2], len[2], stepped[2];
    int slot[2][2];  // [side][env]
    uint32_t ep[2];
    float ret[2][2];  // [side][env]
    alignas(16) floatx4 hpark[4][64];  // hidden state of the side not in its agent phase, [register][lane]
};

// the index map j -> (j + S) mod U of the canonical view on a U-bit mask (an involution: U = 2S)
__device__ __forceinline__ uint32_t view_rot(uint32_t v, int S, int U) {
    return ((v >> S) | (v << S)) & ((1u << U) - 1u);
}

// action bits raw <-> canonical (the same map both ways): 0, 1, 2 kept, 3 / 4 swapped, target bits rotated
__device__ __forceinline__ uint32_t view_avail(uint32_t av, int S, int U) {
    return (av & 7u) | (((av >> 3) & 1u) << 4) | (((av >> 4) & 1u) << 3) | (view_rot(av >> MLG_ACT_BASE, S, U) << MLG_ACT_BASE);
}

// action index raw <-> canonical (the same map both ways); pa in [0, MLG_ACT_BASE + U)
__device__ __forceinline__ int view_action(int pa, int S, int U) {
    if (pa == 3) return 4;
    if (pa == 4) return 3;
    if (pa >= MLG_ACT_BASE) {
        const int j = pa - MLG_ACT_BASE + S;
        return MLG_ACT_BASE + (j >= U ? j - U : j);
    }
    return pa;
}

__device__ __forceinline__ void sp_store_mask_row(uint8_t* dst, uint32_t bits, int U) {
    if (U == 16) {  // one 16-byte row (rows of U bytes: 16-byte aligned when U == 16)
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            w[q] = ((bits >> (4 * q)) & 1u) | (((bits >> (4 * q + 1)) & 1u) << 8) | (((bits >> (4 * q + 2)) & 1u) << 16) |
                   (((bits >> (4 * q + 3)) & 1u) << 24);
        *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int j = 0; j < U; ++j) dst[j] = (uint8_t)((bits >> j) & 1u);
    }
}

// pre-transition data of step t for env e (lanes (e, u)): both sides' batch rows and LDS copies, each in its view
__device__ inline void sp_observe(SpLds& S, const EnvTables& T, const EnvMasks& M, const RoArgs& a,
                                  const MlgEntityBatch& bh, const MlgEntityBatch& ba, int e, int u, bool active, int t) {
    const bool me = active && u < a.U;
    // obs-mask and target bits of unit u: the units j split between the two half-waves, ORed by a permlane32 swap
    // (refil.hip ro_observe; all 64 lanes take part)
    uint32_t om_all, tb_all;
    {
        int pk[16];
        load16(S.pk[e], pk);
        const int pu = S.pk[e][u];
        const bool upper = (threadIdx.x & 32) != 0;
        const int xu = pkx(pu), yu = pky(pu);
        uint32_t om = 0u, tb, kb, ka, ke;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int j = (upper ? 8 : 0) + k;
            const int p = upper ? pk[8 + k] : pk[k];
            const int dx = pkx(p) - xu, dy = pky(p) - yu;
            om |= (uint32_t)(j < M.U && (pkh(p) <= 0 || dx * dx + dy * dy > MLG_SIGHT2)) << j;
        }
        unit_scan<8>(M, pk, u, pu, upper, tb, kb, ka, ke);
        const auto so = __builtin_amdgcn_permlane32_swap(om, om, false, false);
        const auto st = __builtin_amdgcn_permlane32_swap(tb, tb, false, false);
        om_all = om | (upper ? so[0] : so[1]);
        tb_all = tb | (upper ? st[0] : st[1]);
        if (pkh(pu) <= 0) om_all = (1u << M.U) - 1u;  // a dead unit sees nothing
    }
    if (me) {
        const int pu = S.pk[e][u];
        const int uv = u < a.S ? u + a.S : u - a.S;  // index of unit u in the away view
        const int64_t rh = S.slot[0][e] * (int64_t)bh.T1 + t, ra = S.slot[1][e] * (int64_t)ba.T1 + t;
        float f[8];
        entity_feat(T, pkx(pu), pky(pu), pkh(pu), u, a.inv_p, f);
        float* eh = bh.entities + (rh * a.U + u) * a.ED;
        float* ea = ba.entities + (ra * a.U + uv) * a.ED;
        const bool alive = pkh(pu) > 0;
        for (int k = 0; k < 8; ++k) {
            float g = f[k];
            if (alive && k == 1) g = (float)(M.grid - 1 - pkx(pu)) * a.inv_p;
            if (alive && k == 4) g = 1.f - f[4];
            S.feat[0][e][u][k] = f[k];
            S.feat[1][e][uv][k] = g;
            if (k < a.ED) {
                eh[k] = f[k];
                ea[k] = g;
            }
        }
        const uint32_t bits = om_all, vbits = view_rot(om_all, a.S, a.U);
        sp_store_mask_row(bh.obs_mask + (rh * a.U + u) * a.U, bits, a.U);
        sp_store_mask_row(ba.obs_mask + (ra * a.U + uv) * a.U, vbits, a.U);
        S.om[0][e][u] = bits;
        S.om[1][e][uv] = vbits;
        bh.entity_mask[rh * a.U + u] = (uint8_t)!alive;
        ba.entity_mask[ra * a.U + uv] = (uint8_t)!alive;
        {
            const uint32_t raw = !alive ? 1u
                                        : (((uint32_t)(pky(pu) + 1 < M.grid) << 1) | ((uint32_t)(pky(pu) - 1 >= 0) << 2) |
                                           ((uint32_t)(pkx(pu) + 1 < M.grid) << 3) | ((uint32_t)(pkx(pu) - 1 >= 0) << 4) |
                                           (tb_all << MLG_ACT_BASE));
            const int side = u >= a.S, n = u - side * a.S;
            const uint32_t av = side ? view_avail(raw, a.S, a.U) : raw;
            int32_t* ag = (side ? ba.avail + (ra * a.NA + n) * a.A : bh.avail + (rh * a.NA + n) * a.A);
            for (int k = 0; k < a.A; ++k) ag[k] = (int)((av >> k) & 1u);
            S.av[side][e][n] = av;
        }
        if (u == 0) {
            bh.filled[rh] = 1;
            ba.filled[ra] = 1;
        }
    }
    const uint64_t bal = __ballot(me && pkh(S.pk[e][u]) <= 0);
    if (active && u == 0) {
        const uint32_t m = (uint32_t)((bal >> (16 * e)) & 0xFFFFu);
        S.em[0][e] = m;
        S.em[1][e] = view_rot(m, a.S, a.U);
    }
}

// Workgroup = SP_WAVES waves; every wave owns two envs for the whole episode (no cross-wave dependency).
constexpr int SP_WAVES = 4;
struct SpShared {
    SpLds S[SP_WAVES];
};

struct SpArgs {
    float eps[2];
    int la;  // entity_last_action: the side's previous actions as one-hot columns of its agents' entity rows
    int test_mode;
};

template <int KC1>
__global__ void __launch_bounds__(64 * SP_WAVES)
    refil_rollout_selfplay_kernel(MlgEntityEnvSpec spec, MlgEnvState st, RAgent L, const float* __restrict__ Ph,
                                  const float* __restrict__ Pa, MlgEntityBatch bh, MlgEntityBatch ba, MlgRunInfo info,
                                  RoArgs a, SpArgs sa) {
    extern __shared__ __attribute__((aligned(16))) float sp_smem[];
    SpShared& SH = *reinterpret_cast<SpShared*>(sp_smem);
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    SpLds& S = SH.S[wave];
    const int lane = threadIdx.x & 63;
    const int e = (lane >> 4) & 1, u = lane & 15;
    const bool env_lane = lane < 32;
    const int b0 = (blockIdx.x * SP_WAVES + wave) * 2;
    const MlgEnvSpec& sp = spec.base;
    if (lane < NE) {
        const bool in = lane < a.U;
        S.team[lane] = in ? sp.team[lane] : 0;
        S.role[lane] = in ? sp.role[lane] : 0;
        S.melee[lane] = in ? sp.melee[lane] : 0;
        S.agent[lane] = in ? lane + 1 : 0;
    }
    for (int i = lane; i < 16 * LDX; i += 64) S.o[i] = 0.f;
    if (lane < 2) {
        const int b = b0 + lane;
        const bool in = b < a.B;
        S.status[lane] = in ? 0 : 2;
        S.len[lane] = 0;
        S.ret[0][lane] = 0.f;
        S.ret[1][lane] = 0.f;
        S.stepped[lane] = 0;
        S.slot[0][lane] = in ? (int)ro_slot(bh, b) : 0;
        S.slot[1][lane] = in ? (int)ro_slot(ba, b) : 0;
        S.ep[lane] = in ? st.episode[b] : 0u;
    }
    if (lane < 32) S.pact[lane >> 4][(lane >> 3) & 1][lane & 7] = 0;
    wave_sync();
    EnvTables T;
    T.team = S.team;
    T.role = S.role;
    T.melee = S.melee;
    T.agent = S.agent;
    T.U = a.U;
    T.grid = sp.grid;
    T.episode_limit = sp.episode_limit;
    T.stochastic = sp.stochastic;
    EnvMasks M;
    M.team1 = M.healer = M.tank = M.melee = 0;
    for (int j = 0; j < a.U; ++j) {
        M.team1 |= (uint32_t)(S.team[j] != 0) << j;
        M.healer |= (uint32_t)(S.role[j] == 1) << j;
        M.tank |= (uint32_t)(S.role[j] == 0) << j;
        M.melee |= (uint32_t)(S.melee[j] != 0) << j;
    }
    M.U = a.U;
    M.grid = sp.grid;
    // ---- reset (§3b: the same k for both teams) ----
    const int b = b0 + e;
    const bool live = env_lane && b < a.B;
    if (live && u < a.U) {
        const uint64_t key = mlg_env_key(sp.seed, b);
        const uint32_t ep = S.ep[e];
        const int k = entity_team_k(key, ep, a.kmin, a.kmax);
        const int tf = S.team[u] ? a.S : 0;
        int xx, yy, hh;
        env_spawn_xyh(T, key, ep, u, tf, a.S, xx, yy, hh);
        if (u - tf >= k) hh = 0;
        S.x[e][u] = xx;
        S.y[e][u] = yy;
        S.hp[e][u] = hh;
        S.pk[e][u] = pk_pack(xx, yy, hh);
    }
    if (env_lane && u >= a.U) S.pk[e][u] = 0;
    wave_sync();
    sp_observe(S, T, M, a, bh, ba, e, u, live, 0);
    wave_sync();
    // hidden state of the side whose agent phase runs next; the other side's is parked in the wave's LDS (lane-private
    // 16-byte slots, conflict-free). The two swap after every agent phase, so after both sides of a step h is the home
    // side's again: one loop body for both sides (no second copy of the agent code), and the agent phase keeps the
    // register budget of refil.hip's kernel instead of spilling 16 more live VGPRs to scratch.
    floatx4 h[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        h[i] = floatx4{0.f, 0.f, 0.f, 0.f};
        S.hpark[i][lane] = h[i];
    }
    uint64_t rows = 0;
    const int col = lane & 15, g = lane >> 4;
    for (int t = 0;; ++t) {
        if (S.status[0] == 2 && S.status[1] == 2) break;
#pragma nounroll
        for (int side = 0; side < 2; ++side) {
            // opaque per-iteration copy of the weight pointer: keeps the compiler from hoisting the (loop-invariant)
            // weight loads of the step out of the episode loop into registers (refil.hip)
            int64_t zoff = 0;
            asm volatile("" : "+s"(zoff));
            const float* __restrict__ Pw = (side ? Pa : Ph) + zoff;
            // ---- agent phase of this side: EntityMAC.forward(t) + epsilon-greedy for both envs ----
            for (int ee = 0; ee < 2; ++ee) {
                if (S.status[ee] == 2) continue;
                // fc1 B operand: lane (entity j = col of the side's view, g) holds inputs k = 16 kc + 4 g + r
                floatx4 xin[KC1];
                const int j = col;
#pragma unroll
                for (int kc = 0; kc < KC1; ++kc)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int k = kc * 16 + 4 * g + r;
                        float v = 0.f;
                        if (j < a.U) {
                            if (k < a.ED) v = S.feat[side][ee][j][k < 8 ? k : 0];
                            else if (sa.la && k < a.ED + a.A && j < a.NA && t > 0 && S.pact[side][ee][j] == k - a.ED) v = 1.f;
                        }
                        xin[kc][r] = v;
                    }
                entity_block_reg<KC1>(Pw, L, xin, S.q, S.kv, S.om[side][ee], a.NA, a.U, S.o + ee * NAS * LDX, lane);
                rows += (uint64_t)a.NA;
            }
            // tile row r = env (r >> 3), agent (r & 7); dead = agent entity masked
            uint32_t dead = 0;
            for (int ee = 0; ee < 2; ++ee) {
                uint32_t m = S.em[side][ee] & ((1u << a.NA) - 1u);
                m |= ~((1u << a.NA) - 1u) & 0xFFu;  // padding rows >= n_agents
                dead |= (m & 0xFFu) << (8 * ee);
            }
            agent_tile_post_b16(Pw, L, S.o, dead, h, lane);
            // fc3 + masked argmax + epsilon-greedy
            const int re = col >> 3, rn = col & 7;
            const uint32_t avm = (rn < a.NA) ? S.av[side][re][rn] : 1u;
            ArgmaxState as{-INFINITY, 1 << 30};
            Split3 hs3[2];  // fc3 as split-bf16 (wsp tiles 24-25; Ap <= 32 host-checked)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) hs3[kk] = split3(h[2 * kk], h[2 * kk + 1]);
            for (int at = 0; at < L.Ap / 16; ++at) {
                floatx4 q;
                {
                    const u32x4* ws = reinterpret_cast<const u32x4*>(Pw + L.wsp) + lane;
                    bf16x8 w[6];
#pragma unroll
                    for (int i = 0; i < 6; ++i) w[i] = __builtin_bit_cast(bf16x8, ws[((REFIL_WSP_W3 + at) * 6 + i) * 64]);
                    q = ld4(Pw + L.b3 + at * 16 + 4 * g);
#pragma unroll
                    for (int kk = 0; kk < 2; ++kk) {
                        Split3 a3;
                        a3.p[0] = w[kk * 3];
                        a3.p[1] = w[kk * 3 + 1];
                        a3.p[2] = w[kk * 3 + 2];
                        q = mfma_x6(a3, hs3[kk], q);
                    }
                    if ((dead >> (lane & 15)) & 1u) q = floatx4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ac = at * 16 + 4 * g + r;
                    if (ac >= a.A) continue;
                    const float v = ((avm >> ac) & 1u) ? q[r] : -INFINITY;
                    if (amax_better(v, ac, as.bv, as.bi)) { as.bv = v; as.bi = ac; }
                }
            }
            int act = argmax_reduce(as);
            const int bb = b0 + re;
            const float eps = side ? sa.eps[1] : sa.eps[0];
            if (g == 0 && rn < a.NA && S.status[re] != 2) {
                if (!sa.test_mode && eps > 0.f) {
                    // the RNG stream index is the global agent index: home n, away S + n (mlg_rollout_selfplay)
                    const uint32_t stream = (uint32_t)(side * a.NA + rn);
                    const uint64_t key = mlg_env_key(sp.seed, bb);
                    const uint64_t r1 = mlg_rng(key, mlg_ctr(S.ep[re], (uint32_t)t, MLG_PURPOSE_EPS, stream));
                    if (mlg_u01(r1) < eps) {
                        const uint64_t r2 = mlg_rng(key, mlg_ctr(S.ep[re], (uint32_t)t, MLG_PURPOSE_RAND, stream));
                        const int na = __popc(avm);
                        if (na == 0) {
                            act = 0;
                        } else {  // the k-th available action in the side's view order
                            const int k = (int)(((r2 >> 40) * (uint64_t)na) >> 24);
                            uint32_t m = avm;
                            for (int i = 0; i < k; ++i) m &= m - 1;
                            act = __ffs((int)m) - 1;
                        }
                    }
                }
                S.pact[side][re][rn] = act;
                const int T1 = side ? ba.T1 : bh.T1;
                const int64_t off = ((int64_t)S.slot[side][re] * T1 + t) * a.NA + rn;
                int64_t* ag = side ? ba.actions : bh.actions;
                ag[off] = act;
                float* oh = (side ? ba.actions_onehot : bh.actions_onehot) + off * a.A;
                if (side ? ba.full_write : bh.full_write) {
                    for (int k = 0; k < a.A; ++k) oh[k] = k == act ? 1.f : 0.f;
                } else {
                    oh[act] = 1.f;
                }
            }
            wave_sync();
#pragma unroll
            for (int i = 0; i < 4; ++i) {  // lane-private slots: a lane reads back only what it stored itself
                const floatx4 other = S.hpark[i][lane];
                S.hpark[i][lane] = h[i];
                h[i] = other;
            }
        }
        // ---- env phase: both teams execute their policies' validated actions (§3b') ----
        const bool stepping = env_lane && S.status[e] == 0;
        int pk[16];
        load16(S.pk[e], pk);
        const int pu = S.pk[e][u];
        {  // lanes 32-63 (no env of their own) mirror unit u of env e and scan the upper half of the units j
            uint32_t tb, kb, ka, ke;
            unit_scan<8>(M, pk, u, pu, lane >= 32, tb, kb, ka, ke);
            const auto s2 = __builtin_amdgcn_permlane32_swap(tb, tb, false, false);
            tb |= (threadIdx.x & 32) ? s2[0] : s2[1];
            if (stepping && u < a.U) {
                const int side = u >= a.S, n = u - side * a.S;
                int pa = S.pact[side][e][n];
                const bool in = pa >= 0 && pa < MLG_ACT_BASE + a.U;
                if (in && side) pa = view_action(pa, a.S, a.U);  // the raw image of the away side's choice
                const uint32_t av = pkh(pu) <= 0 ? 1u
                                                 : (((uint32_t)(pky(pu) + 1 < M.grid) << 1) |
                                                    ((uint32_t)(pky(pu) - 1 >= 0) << 2) |
                                                    ((uint32_t)(pkx(pu) + 1 < M.grid) << 3) |
                                                    ((uint32_t)(pkx(pu) - 1 >= 0) << 4) | (tb << MLG_ACT_BASE));
                S.act[e][u] = (in && ((av >> pa) & 1u)) ? pa : 0;
            }
        }
        wave_sync();
        if (stepping && u < a.U) {
            int acts[16];
            load16(S.act[e], acts);
            S.nhp[e][u] = resolve_hp_reg(M, pk, acts, u, pu);
        }
        wave_sync();
        if (stepping && u < a.U && S.hp[e][u] > 0) env_apply_move(S.act[e][u], &S.x[e][u], &S.y[e][u]);
        // per-unit step results as lane ballots (bit 16 e + u): alive after, killed, bits of the hp lost (<= 64)
        uint64_t rw_alive, rw_kill, rw_loss[7];
        {
            const bool v = stepping && u < a.U;
            const int h0 = v ? S.hp[e][u] : 0, h1 = v ? S.nhp[e][u] : 0;
            const int loss = (h0 > 0 && h0 > h1) ? h0 - h1 : 0;
            rw_alive = __ballot(v && h1 > 0);
            rw_kill = __ballot(v && h0 > 0 && h1 == 0);
#pragma unroll
            for (int bb = 0; bb < 7; ++bb) rw_loss[bb] = __ballot((loss >> bb) & 1);
        }
        if (env_lane && u == 0) {
            const int stt = S.status[e];
            S.stepped[e] = 0;
            const int64_t sh = (int64_t)S.slot[0][e] * bh.T1 + t, sl = (int64_t)S.slot[1][e] * ba.T1 + t;
            if (stt == 1) {  // final action recorded; env done
                S.status[e] = 2;
                if (bh.full_write) {
                    bh.reward[sh] = 0.f;
                    bh.terminated[sh] = 0;
                }
                if (ba.full_write) {
                    ba.reward[sl] = 0.f;
                    ba.terminated[sl] = 0;
                }
            } else if (stt == 0) {
                int alive[2] = {0, 0}, lost[2] = {0, 0}, kills[2] = {0, 0};
                const uint32_t t1 = M.team1 & ((1u << a.U) - 1u);
                const uint32_t am = (uint32_t)(rw_alive >> (16 * e)) & 0xFFFFu, km = (uint32_t)(rw_kill >> (16 * e)) & 0xFFFFu;
                alive[0] = __builtin_popcount(am & ~t1);
                alive[1] = __builtin_popcount(am & t1);
                kills[0] = __builtin_popcount(km & t1);  // team-1 units killed: credited to team 0
                kills[1] = __builtin_popcount(km & ~t1);
#pragma unroll
                for (int bb = 0; bb < 7; ++bb) {
                    const uint32_t lm = (uint32_t)(rw_loss[bb] >> (16 * e)) & 0xFFFFu;
                    lost[0] += __builtin_popcount(lm & ~t1) << bb;
                    lost[1] += __builtin_popcount(lm & t1) << bb;
                }
                const int done = alive[0] == 0 || alive[1] == 0 || t + 1 >= sp.episode_limit;
                const int w0 = alive[1] == 0 && alive[0] > 0, w1 = alive[0] == 0 && alive[1] > 0;
                const float r0 = (float)(lost[1] + 10 * kills[0] + 200 * w0) * 0.0625f;  // home = team 0
                const float r1 = (float)(lost[0] + 10 * kills[1] + 200 * w1) * 0.0625f;  // away = team 1
                bh.reward[sh] = r0;
                bh.terminated[sh] = (uint8_t)done;
                ba.reward[sl] = r1;
                ba.terminated[sl] = (uint8_t)done;
                S.ret[0][e] += r0;
                S.ret[1][e] += r1;
                S.stepped[e] = 1;
                if (done) {
                    S.status[e] = 1;
                    S.len[e] = t + 1;
                    const int bb2 = b0 + e;
                    info.won[2 * bb2] = w0;
                    info.won[2 * bb2 + 1] = w1;
                    info.draw[bb2] = !w0 && !w1;
                }
            }
        }
        wave_sync();
        const bool stepped = env_lane && S.stepped[e];
        if (stepped && u < a.U) {
            S.hp[e][u] = S.nhp[e][u];
            S.pk[e][u] = pk_pack(S.x[e][u], S.y[e][u], S.nhp[e][u]);
        }
        wave_sync();
        sp_observe(S, T, M, a, bh, ba, e, u, stepped, t + 1);
        wave_sync();
    }
    // ---- finish: run summary, env state, full-write tails ----
    if (live && u == 0) {
        info.ep_len[b] = S.len[e];
        info.ret[b] = S.ret[0][e];
        if (info.ret_away) info.ret_away[b] = S.ret[1][e];
        st.t[b] = S.len[e];
        st.episode[b] = S.ep[e] + 1u;
    }
    if (live && u < a.U) {
        st.x[(int64_t)b * a.U + u] = S.x[e][u];
        st.y[(int64_t)b * a.U + u] = S.y[e][u];
        st.hp[(int64_t)b * a.U + u] = S.hp[e][u];
    }
    for (int ee = 0; ee < 2; ++ee) {
        if (b0 + ee >= a.B) continue;
        if (bh.full_write) ro_zero_tail(bh, a, S.slot[0][ee], S.len[ee] + 1, lane);
        if (ba.full_write) ro_zero_tail(ba, a, S.slot[1][ee], S.len[ee] + 1, lane);
    }
    if (info.agent_rows && lane == 0) atomicAdd((unsigned long long*)info.agent_rows, (unsigned long long)rows);
}

// The launch mlg_refil_rollout_selfplay makes for a spec and one side's agent dims: decided here for the entry point
// and for mlg_refil_rollout_selfplay_describe, so the query cannot drift from the launch (the contract of
// plan_refil_rollout, refil.hip).
struct RefilSelfplayPlan {
    const char* name;  // "sp-ro2/kcK": two envs per wave, entity input width 16 K
    int kc;
    size_t lds_bytes;
};

#define SP_NAME "refil_rollout_selfplay"

int plan_refil_selfplay(const MlgEntityEnvSpec* spec, const MlgRefilDims* d, RefilSelfplayPlan* plan) {
    MLG_REQUIRE(spec != nullptr && d != nullptr, SP_NAME ": null argument");
    if (check_refil_dims(d)) return mlg::fail(SP_NAME ": %s", std::string(mlg::last_error()).c_str());
    const MlgEnvSpec& sp = spec->base;
    const int S = sp.U / 2;
    MLG_REQUIRE(sp.U >= 2 && sp.U % 2 == 0 && sp.U <= NE && S <= NAS, SP_NAME ": U=%d unsupported (even, <= 16)", sp.U);
    bool two = sp.n_policy_teams == 2 && sp.policy_team == 0 && sp.scripted[0] == 0 && sp.scripted[1] == 0 &&
               sp.n_agents == 2 * S;
    for (int u = 0; two && u < sp.U; ++u) two = sp.agent_unit[u] == u && sp.team[u] == (u >= S);
    MLG_REQUIRE(two,
                SP_NAME ": the spec is not the two-policy entity scenario (n_policy_teams=%d policy_team=%d "
                        "scripted=[%d, %d] n_agents=%d; need 2, 0, [0, 0], %d agents with agent_unit[a] = a, home units "
                        "0..%d, away units %d..%d)",
                sp.n_policy_teams, sp.policy_team, sp.scripted[0], sp.scripted[1], sp.n_agents, 2 * S, S - 1, S,
                2 * S - 1);
    MLG_REQUIRE(d->n_agents == S && d->n_entities == sp.U && d->entity_shape == 8 && d->n_actions == MLG_ACT_BASE + sp.U &&
                    sp.n_actions == MLG_ACT_BASE + sp.U,
                SP_NAME ": dims (n_agents=%d n_entities=%d entity_shape=%d n_actions=%d) do not describe one side of the "
                        "env (S=%d, U=%d)",
                d->n_agents, d->n_entities, d->entity_shape, d->n_actions, S, sp.U);
    MLG_REQUIRE(spec->min_agents >= 1 && spec->min_agents <= spec->max_agents && spec->max_agents <= S,
                SP_NAME ": min_agents=%d max_agents=%d (slots %d)", spec->min_agents, spec->max_agents, S);
    MLG_REQUIRE(sp.grid >= 1 && sp.grid <= 255, SP_NAME ": grid=%d unsupported (1..255)", sp.grid);
    const RAgent L = make_ragent(refil_d0(d), d->n_actions);
    const int kc = L.K1 <= 16 ? 1 : (L.K1 <= 32 ? 2 : 3);
    static const char* const names[3] = {"sp-ro2/kc1", "sp-ro2/kc2", "sp-ro2/kc3"};
    *plan = RefilSelfplayPlan{names[kc - 1], kc, sizeof(SpShared)};
    return 0;
}

bool batch_complete(const MlgEntityBatch& bt) {
    return bt.entities && bt.obs_mask && bt.entity_mask && bt.actions && bt.avail && bt.reward && bt.terminated &&
           bt.actions_onehot && bt.filled;
}

}  // namespace

extern "C" int mlg_refil_rollout_selfplay_describe(const MlgEntityEnvSpec* spec, const MlgRefilDims* d, char* name,
                                                   int32_t name_cap, int64_t* lds_bytes) {
    MLG_REQUIRE(name && name_cap > 0 && lds_bytes, SP_NAME "_describe: null output");
    RefilSelfplayPlan plan;
    if (int rc = plan_refil_selfplay(spec, d, &plan)) return rc;
    MLG_REQUIRE((size_t)name_cap > strlen(plan.name), SP_NAME "_describe: name buffer of %d bytes too small", name_cap);
    strcpy(name, plan.name);
    *lds_bytes = (int64_t)plan.lds_bytes;
    return 0;
}

extern "C" int mlg_refil_rollout_selfplay(const MlgEntityEnvSpec* spec, MlgEnvState* st, const MlgRefilDims* d,
                                          const float* home_packed, const float* away_packed, MlgEntityBatch* home,
                                          MlgEntityBatch* away, MlgRunInfo* info, float eps_home, float eps_away,
                                          int32_t test_mode, void* stream) {
    MLG_REQUIRE(spec && st && d && home_packed && away_packed && home && away && info, SP_NAME ": null argument");
    RefilSelfplayPlan plan;
    if (int rc = plan_refil_selfplay(spec, d, &plan)) return rc;
    MLG_REQUIRE(mlg::aligned16(home_packed) && mlg::aligned16(away_packed),
                SP_NAME ": the packed weight blocks must be 16-byte aligned (home %p, away %p)", (const void*)home_packed,
                (const void*)away_packed);
    const MlgEnvSpec& sp = spec->base;
    const int S = sp.U / 2;
    const MlgEntityBatch &bh = *home, &ba = *away;
    MLG_REQUIRE(batch_complete(bh), SP_NAME ": home batch has null tensors");
    MLG_REQUIRE(batch_complete(ba), SP_NAME ": away batch has null tensors");
    MLG_REQUIRE(st->B == bh.B && st->B == ba.B && bh.T1 >= sp.episode_limit + 1 && ba.T1 >= sp.episode_limit + 1,
                SP_NAME ": B=%d/%d/%d T1=%d/%d (episode_limit %d)", st->B, bh.B, ba.B, bh.T1, ba.T1, sp.episode_limit);
    MLG_REQUIRE(st->x && st->y && st->hp && st->t && st->episode, SP_NAME ": env state has null buffers");
    MLG_REQUIRE(info->ep_len && info->ret && info->won && info->draw, SP_NAME ": run info has null buffers");
    if (bh.B == 0) return 0;
    int p = 1;
    while (p < sp.grid) p <<= 1;
    RoArgs a{sp.U, S, d->n_actions, d->entity_shape, S, spec->min_agents, spec->max_agents, bh.B, 1.0f / (float)p};
    SpArgs sa{{test_mode ? 0.f : eps_home, test_mode ? 0.f : eps_away}, d->entity_last_action ? 1 : 0, test_mode ? 1 : 0};
    const RAgent L = make_ragent(refil_d0(d), d->n_actions);
    auto kern = plan.kc == 1 ? refil_rollout_selfplay_kernel<1>
                             : (plan.kc == 2 ? refil_rollout_selfplay_kernel<2> : refil_rollout_selfplay_kernel<3>);
    const size_t lds = plan.lds_bytes;
    static bool attr_set[3] = {false, false, false};
    const int ki = plan.kc - 1;
    if (!attr_set[ki]) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds);
        if (e != hipSuccess) return mlg::fail(SP_NAME ": LDS %zu B: %s", lds, hipGetErrorString(e));
        attr_set[ki] = true;
    }
    const int per_block = 2 * SP_WAVES;
    hipLaunchKernelGGL(kern, dim3((unsigned)((bh.B + per_block - 1) / per_block)), dim3(64 * SP_WAVES), lds,
                       (hipStream_t)stream, *spec, *st, L, home_packed, away_packed, bh, ba, *info, a, sa);
    return mlg::check_launch(SP_NAME);
}
