// refil_ro4.inc -- the REFIL rollout with four envs per wave (included by refil.hip inside its anonymous namespace).
//
// ParallelStepper.run over the entity env variant with EntityMAC acting, the same semantics as
// refil_rollout_kernel (refil.hip; parallel_stepper.py:106-216, entity_controller.py:11-30,
// entity_rnn_agent.py:32-65, action_selectors.py:44-62), restructured for the CU:
//
//   * a wave owns FOUR envs for the whole episode and a workgroup of four waves (one per SIMD) 16 envs, so 4096 envs
//     are one round of 256 workgroups (the two-env kernel needs two rounds: each env slot played two episodes back
//     to back and the kernel followed the longest pair);
//   * envs 2p, 2p + 1 form pair p: their entity blocks (fc1, in_trans) run on the same weight registers (one stream
//     of pre-split weights from L2 for two 16-entity tiles, two independent MFMA chains per output tile), and their
//     2 x 8 agent rows form agent tile p; out_trans, fc2, GRUCell and fc3 run both tiles on the same weight
//     registers, so every weight stage loaded from L2 feeds two tiles (the two-env kernel: one);
//   * GRU gates on v_exp_f32 / v_rcp_f32 (fast_sigmoid / fast_tanh, as the v7 rollout: the recorded actions are the
//     fp32 oracle's argmax within the 1e-4 Q tolerance of the parity tests);
//   * env phase: lane = (env, unit), 4 envs x 16 units fill the wave (no idle half-wave);
//   * one-hot action rows written by all 64 lanes from the LDS action table (6 stores per lane, not 21).
// Env arithmetic, masks, bookkeeping and epsilon draws are the two-env kernel's (bit-exact vs oracle/env_ref.c).

constexpr int R4_WAVES = 4;  // one wave per SIMD
constexpr int R4_ENVS = 4;   // envs per wave = 2 agent tiles of 2 envs x 8 agent rows

struct R4Lds {
    float q[2][NAS * LDX];   // queries (agent rows) of the current pair's two envs
    float kv[2][NE * LDKV];  // keys | values of the current pair's two envs
    float o[2][16 * LDX];    // attention outputs = out_trans input rows of agent tile p (env 2p rows 0-7, 2p+1 8-15)
    float feat[R4_ENVS][NE][8];
    uint32_t om[R4_ENVS][NE];
    uint32_t av[R4_ENVS][NAS];
    uint32_t em[R4_ENVS];
    int x[R4_ENVS][NE], y[R4_ENVS][NE], hp[R4_ENVS][NE], act[R4_ENVS][NE], nhp[R4_ENVS][NE];
    int pk[R4_ENVS][NE];  // packed unit states x | y << 8 | hp << 16
    int pact[R4_ENVS][NAS];
    int status[R4_ENVS], len[R4_ENVS], slot[R4_ENVS], stepped[R4_ENVS];
    uint32_t ep[R4_ENVS];
    float ret[R4_ENVS];
};

struct R4Shared {
    int team[NE], role[NE], melee[NE], agent[NE];
    R4Lds S[R4_WAVES];
};

// Weight and bias reads through one buffer resource over the packed agent block: the per-lane byte offset (lane * 16
// for the pre-split MFMA operands, 16 g for a bias quad) in a VGPR, the register's byte offset wave-uniform (SGPR /
// immediate). Replaces a 64-bit VGPR address per load and one 64-bit SGPR base per weight section (the two-env
// kernel's address arithmetic: ~900 v_readlane of spilled SGPRs in the unrolled step).
// Every byte offset goes through an opaque zero (asm volatile, once per load): otherwise the compiler hoists the
// ~850 loop-invariant SGPR offsets of the unrolled step out of the episode loop and spills them.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t r4_rsrc(const float* P) { return mlg_rsrc(P); }
__device__ __forceinline__ int opaque_so(int v) {
    asm volatile("" : "+s"(v));
    return v;
}
// register `reg` (1 KB: 64 lanes x 16 B) of a pre-split section at float offset `sect`
__device__ __forceinline__ bf16x8 wld(__amdgpu_buffer_rsrc_t rs, int64_t sect, int reg, int lane) {
    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, lane * 16,
                                                                          opaque_so((int)(sect * 4)) + reg * 1024, 0));
}
// bias quad: floats off + mt * 16 + 4 g .. + 3 (the D layout's four output features of the lane)
__device__ __forceinline__ floatx4 bld(__amdgpu_buffer_rsrc_t rs, int64_t off, int mt, int lane) {
    return ld4_rs(rs, (lane >> 4) * 16, opaque_so((int)(off * 4)) + mt * 64);
}
template <int MT>
__device__ __forceinline__ void bias_rs(floatx4 (&acc)[MT], __amdgpu_buffer_rsrc_t rs, int64_t off, int lane) {
#pragma unroll
    for (int i = 0; i < MT; ++i) acc[i] = bld(rs, off, i, lane);
}

// pre-transition data of step t for env e, lane (e, u): batch rows and the LDS copies (ro_observe with one env per
// 16 lanes: the unit scans run over all 16 units in the lane)
RO_PHASE void r4_observe(R4Lds& S, const EnvTables& T, const EnvMasks& M, const RoArgs& a, const MlgEntityBatch& bt,
                         int e, int u, bool active, int t) {
    const bool me = active && u < a.U;
    int pk[16];
    load16(S.pk[e], pk);
    const int pu = S.pk[e][u];
    const uint32_t om = om_bits(M, pk, u, pu);
    if (me) {
        const int64_t row = (S.slot[e] * (int64_t)bt.T1 + t);
        float f[8];
        entity_feat(T, pkx(pu), pky(pu), pkh(pu), u, a.inv_p, f);
        float* eg = bt.entities + (row * a.U + u) * a.ED;
        *reinterpret_cast<floatx4*>(&S.feat[e][u][0]) = floatx4{f[0], f[1], f[2], f[3]};
        *reinterpret_cast<floatx4*>(&S.feat[e][u][4]) = floatx4{f[4], f[5], f[6], f[7]};
        for (int k = 0; k < a.ED; ++k) eg[k] = f[k];
        uint8_t* omg = bt.obs_mask + (row * a.U + u) * a.U;
        if (a.U == 16) {  // one 16-byte row (rows of U bytes: 16-byte aligned when U == 16)
            uint32_t w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                w[q] = ((om >> (4 * q)) & 1u) | (((om >> (4 * q + 1)) & 1u) << 8) | (((om >> (4 * q + 2)) & 1u) << 16) |
                       (((om >> (4 * q + 3)) & 1u) << 24);
            *reinterpret_cast<uint4*>(omg) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            for (int j = 0; j < a.U; ++j) omg[j] = (uint8_t)((om >> j) & 1u);
        }
        S.om[e][u] = om;
        bt.entity_mask[row * a.U + u] = (uint8_t)(pkh(pu) <= 0);
        if (u < a.NA) {
            const uint32_t av = avail_bits(M, pk, u, pu);
            int32_t* ag = bt.avail + (row * a.NA + u) * a.A;
            for (int k = 0; k < a.A; ++k) ag[k] = (int)((av >> k) & 1u);
            S.av[e][u] = av;
        }
        if (u == 0) bt.filled[row] = 1;
    }
    const uint64_t bal = __ballot(me && pkh(pu) <= 0);
    if (active && u == 0) S.em[e] = (uint32_t)((bal >> (16 * e)) & 0xFFFFu);
}

// Entity blocks of pair p (envs 2p, 2p + 1) at step t: entity inputs -> fc1 -> in_trans (split-bf16, one weight
// stream for both envs) -> q / k | v in LDS -> attention per env into the pair's agent-tile rows S.o[p].
// LIVE: which envs of the pair still run (bit 0: env 2p, bit 1: env 2p + 1). A finished env's entity tile is skipped
// (its fc1 / in_trans MFMA chains, q / k | v rows and attention): its agent rows are never read again (no action is
// recorded for it, and the MFMA columns of the pair's other env do not depend on them).
template <int KC1, int LIVE>
RO_PHASE void r4_entity_pair(const float* __restrict__ P, const RAgent& L, R4Lds& S, int p, const RoArgs& a, int t,
                             int lane, RStamps& stp) {
    static_assert(KC1 == 2, "r4 rollout: entity input width 17..32 (ED = 8, A <= 24)");
    constexpr bool LV[2] = {(LIVE & 1) != 0, (LIVE & 2) != 0};
    const int col = lane & 15, g = lane >> 4;
    const __amdgpu_buffer_rsrc_t rs = r4_rsrc(P);
    // fc1 B operand: lane (entity j = col, g) holds inputs k = 16 kc + 4 g + r: features k < 8 (ED = 8), then the
    // last-action one-hot k - 8 (agents only, zeros at t = 0)
    Split3 xs[2];
    {
        floatx4 xin[2][2];
#pragma unroll
        for (int ee = 0; ee < 2; ++ee) {
            if (!LV[ee]) continue;
            const int e = 2 * p + ee;
            const int la = (col < a.NA && t > 0) ? S.pact[e][col & 7] : -1;
#pragma unroll
            for (int kc = 0; kc < 2; ++kc) {
                if (kc == 0 && g < 2) {
                    xin[ee][kc] = *reinterpret_cast<const floatx4*>(&S.feat[e][col][4 * g]);
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) xin[ee][kc][r] = (kc * 16 + 4 * g + r - 8 == la) ? 1.f : 0.f;
                }
            }
            xs[ee] = split3(xin[ee][0], xin[ee][1]);
        }
    }
    floatx4 x1[2][4];
    bf16x8 wb[2][18];  // in_trans stages: [tile in stage * 6 + kk * 3 + piece]
    auto load = [&](int stg, bf16x8 (&w)[18]) {
#pragma unroll
        for (int i = 0; i < 18; ++i) w[i] = wld(rs, L.wsp, stg * 18 + i, lane);
    };
    {
        bf16x8 w[12];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int pc = 0; pc < 3; ++pc)
                w[mt * 3 + pc] = wld(rs, L.wsp, (REFIL_WSP_W1 + mt) * 6 + pc, lane);
#pragma unroll
        for (int ee = 0; ee < 2; ++ee)
            if (LV[ee]) bias_rs<4>(x1[ee], rs, L.b1, lane);
        load(0, wb[0]);  // in_trans' first stage in flight during fc1
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            Split3 wa;
            wa.p[0] = w[mt * 3];
            wa.p[1] = w[mt * 3 + 1];
            wa.p[2] = w[mt * 3 + 2];
#pragma unroll
            for (int ee = 0; ee < 2; ++ee)
                if (LV[ee]) x1[ee][mt] = relu4(mfma_x6(wa, xs[ee], x1[ee][mt]));
        }
    }
    stp.mark(16);
    // in_trans (192 x 64): x1 split once per 32-wide K step, weights streamed in stages of 3 output tiles (the next
    // stage's 18 loads in flight during the current stage's 2 x 36 MFMAs); tiles 0-3 = q (agent rows only), 4-11 k | v
    Split3 x1s[2][2];
#pragma unroll
    for (int ee = 0; ee < 2; ++ee)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
            if (LV[ee]) x1s[ee][kk] = split3(x1[ee][2 * kk], x1[ee][2 * kk + 1]);
#pragma unroll
    for (int stg = 0; stg < 4; ++stg) {
        if (stg + 1 < 4) load(stg + 1, wb[(stg + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        const bf16x8(&w)[18] = wb[stg & 1];
#pragma unroll
        for (int ti = 0; ti < 3; ++ti) {
            const int mt = stg * 3 + ti;
            floatx4 acc[2];
#pragma unroll
            for (int ee = 0; ee < 2; ++ee) acc[ee] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                Split3 wa;
                wa.p[0] = w[ti * 6 + kk * 3 + 0];
                wa.p[1] = w[ti * 6 + kk * 3 + 1];
                wa.p[2] = w[ti * 6 + kk * 3 + 2];
#pragma unroll
                for (int ee = 0; ee < 2; ++ee)
                    if (LV[ee]) acc[ee] = mfma_x6(wa, x1s[ee][kk], acc[ee]);
            }
#pragma unroll
            for (int ee = 0; ee < 2; ++ee) {
                if (!LV[ee]) continue;
                if (mt < 4) {
                    if (col < NAS) st_row(S.q[ee], LDX, mt, acc[ee], lane);
                } else {
                    st_row(S.kv[ee], LDKV, mt - 4, acc[ee], lane);
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    wave_sync();
    stp.mark(17);
#pragma unroll
    for (int ee = 0; ee < 2; ++ee) {
        if (!LV[ee] || S.status[2 * p + ee] == 2) continue;  // finished env of a running pair: its rows are not used
        attn_fwd_half(S.q[ee], LDX, S.kv[ee], S.kv[ee] + EMB, LDKV, S.om[2 * p + ee], a.NA, a.U, S.o[p] + ee * NAS * LDX,
                      LDX, lane);
    }
    wave_sync();
    stp.mark(18);
}

// GRUCell stage st = (output tile st >> 1, K step st & 1) of the pre-split W_ih / W_hh: [mat * 9 + gate * 3 + piece]
__device__ __forceinline__ void r4_gru_load(__amdgpu_buffer_rsrc_t rs, const RAgent& L, int st, bf16x8 (&w)[18], int lane) {
    const int mt = st >> 1, kk = st & 1;
#pragma unroll
    for (int mat = 0; mat < 2; ++mat)
#pragma unroll
        for (int gate = 0; gate < 3; ++gate)
#pragma unroll
            for (int pc = 0; pc < 3; ++pc)
                w[mat * 9 + gate * 3 + pc] = wld(rs, L.gsp, refil_gsp_reg(mat, mt, gate, kk, pc) / 64, lane);
}
// GRUCell on NT agent tiles sharing every weight stage (gru_tile_b16's split-bf16 scheme, fast gates); weight stages
// and bias quads are requested one stage / output tile ahead.
template <int NT>
__device__ inline void r4_gru(const float* __restrict__ P, const RAgent& L, const floatx4 (&x)[NT][4],
                              floatx4 (&h)[NT][4], int lane) {
    const __amdgpu_buffer_rsrc_t rs = r4_rsrc(P);
    Split3 xs[NT][2], hs[NT][2];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            xs[t][kk] = split3(x[t][2 * kk], x[t][2 * kk + 1]);
            hs[t][kk] = split3(h[t][2 * kk], h[t][2 * kk + 1]);
        }
    bf16x8 wb[2][18];
    auto load = [&](int st, bf16x8 (&w)[18]) { r4_gru_load(rs, L, st, w, lane); };
    auto piece3 = [](const bf16x8 (&w)[18], int b) {
        Split3 s;
        s.p[0] = w[b];
        s.p[1] = w[b + 1];
        s.p[2] = w[b + 2];
        return s;
    };
    floatx4 hn[NT][4];
    load(0, wb[0]);
    floatx4 bq[4];  // bias quads of the next output tile, loaded one tile ahead
    auto bias4 = [&](int mt) {
        bq[0] = bld(rs, L.brz, mt, lane);
        bq[1] = bld(rs, L.brz + EMB, mt, lane);
        bq[2] = bld(rs, L.bih + 2 * EMB, mt, lane);
        bq[3] = bld(rs, L.bhh + 2 * EMB, mt, lane);
    };
    bias4(0);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const floatx4 br = bq[0], bz = bq[1], bn = bq[2], bhn = bq[3];
        if (mt + 1 < 4) bias4(mt + 1);
        floatx4 ar[NT], az[NT], ain[NT], ahn[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            ar[t] = br;
            az[t] = bz;
            ain[t] = bn;
            ahn[t] = bhn;
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            const int st = mt * 2 + kk;
            if (st + 1 < 8) load(st + 1, wb[(st + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            const bf16x8(&w)[18] = wb[st & 1];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                ar[t] = mfma_x6(piece3(w, 0), xs[t][kk], ar[t]);
                az[t] = mfma_x6(piece3(w, 3), xs[t][kk], az[t]);
                ain[t] = mfma_x6(piece3(w, 6), xs[t][kk], ain[t]);
                ar[t] = mfma_x6(piece3(w, 9), hs[t][kk], ar[t]);
                az[t] = mfma_x6(piece3(w, 12), hs[t][kk], az[t]);
                ahn[t] = mfma_x6(piece3(w, 15), hs[t][kk], ahn[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float rg = fast_sigmoid(ar[t][r]);
                const float zg = fast_sigmoid(az[t][r]);
                const float ng = fast_tanh(ain[t][r] + rg * ahn[t][r]);
                hn[t][mt][r] = ng + zg * (h[t][mt][r] - ng);
            }
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) h[t][mt] = hn[t][mt];
}

// out_trans (+ post mask) -> fc2 -> ReLU -> GRUCell on NT agent tiles (agent_tile_post_b16 with shared weights).
template <int NT>
RO_PHASE void r4_post(const float* __restrict__ P, const RAgent& L, const float* o0, const float* o1, uint32_t dead0,
                      uint32_t dead1, floatx4 (&h0)[4], floatx4 (&h1)[4], int lane, RStamps& stp) {
    const int col = lane & 15, g = lane >> 4;
    const __amdgpu_buffer_rsrc_t rs = r4_rsrc(P);
    const float* ob[2] = {o0, o1};
    const uint32_t dd[2] = {dead0, dead1};
    auto piece3 = [](const bf16x8 (&w)[24], int b) {
        Split3 s;
        s.p[0] = w[b];
        s.p[1] = w[b + 1];
        s.p[2] = w[b + 2];
        return s;
    };
    floatx4 h[NT][4];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        h[0][mt] = h0[mt];
        if constexpr (NT == 2) h[1][mt] = h1[mt];
    }
    floatx4 x3[NT][4];
    {
        bf16x8 wo[24];  // [tile * 6 + kk * 3 + piece]
#pragma unroll
        for (int i = 0; i < 24; ++i) wo[i] = wld(rs, L.wsp, REFIL_WSP_WOUT * 6 + i, lane);
        Split3 os[NT][2];
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
                os[t][kk] = split3(ld4(ob[t] + col * LDX + 2 * kk * 16 + 4 * g),
                                   ld4(ob[t] + col * LDX + (2 * kk + 1) * 16 + 4 * g));
        floatx4 x2[NT][4];
#pragma unroll
        for (int t = 0; t < NT; ++t) bias_rs<4>(x2[t], rs, L.bout, lane);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int t = 0; t < NT; ++t) x2[t][mt] = mfma_x6(piece3(wo, mt * 6 + kk * 3), os[t][kk], x2[t][mt]);
        stp.mark(19);
        bf16x8 w2[24];
#pragma unroll
        for (int i = 0; i < 24; ++i) w2[i] = wld(rs, L.wsp, REFIL_WSP_W2 * 6 + i, lane);
        Split3 xs[NT][2];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if ((dd[t] >> col) & 1u) {  // post mask (attention.py:75-76)
#pragma unroll
                for (int i = 0; i < 4; ++i) x2[t][i] = floatx4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) xs[t][kk] = split3(x2[t][2 * kk], x2[t][2 * kk + 1]);
            bias_rs<4>(x3[t], rs, L.b2, lane);
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int t = 0; t < NT; ++t) x3[t][mt] = mfma_x6(piece3(w2, mt * 6 + kk * 3), xs[t][kk], x3[t][mt]);
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) x3[t][i] = relu4(x3[t][i]);
    }
    stp.mark(20);
    r4_gru<NT>(P, L, x3, h, lane);
    stp.mark(21);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        h0[mt] = h[0][mt];
        if constexpr (NT == 2) h1[mt] = h[1][mt];
    }
}

// fc3 + masked argmax + epsilon-greedy for NT agent tiles (tile i = pair tp[i]); picks into S.pact, actions into the
// batch. Lanes (col = tile row, g); every 16-lane row group ends with the row's greedy pick (argmax_reduce).
template <int NT>
RO_PHASE void r4_select(const float* __restrict__ P, const RAgent& L, R4Lds& S, const RoArgs& a, const MlgEntityBatch& bt,
                        uint64_t seed, int b0, int p0, uint32_t dead0, uint32_t dead1, const floatx4 (&h0)[4],
                        const floatx4 (&h1)[4], float eps, int test_mode, int t, int lane, RStamps& stp) {
    const int col = lane & 15, g = lane >> 4;
    const int re = col >> 3, rn = col & 7;
    const uint32_t dd[2] = {dead0, dead1};
    ArgmaxState as[NT];
    uint32_t avm[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        as[i] = ArgmaxState{-INFINITY, 1 << 30};
        const int e = 2 * (p0 + i) + re;
        avm[i] = (rn < a.NA) ? S.av[e][rn] : 1u;
    }
    Split3 hs3[NT][2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
        hs3[0][kk] = split3(h0[2 * kk], h0[2 * kk + 1]);
        if constexpr (NT == 2) hs3[1][kk] = split3(h1[2 * kk], h1[2 * kk + 1]);
    }
    const __amdgpu_buffer_rsrc_t rs = r4_rsrc(P);
    bf16x8 w3[2][6];  // both output tiles' weights in flight together (Ap <= 32)
    floatx4 b3q[2];
#pragma unroll
    for (int at = 0; at < 2; ++at) {
        if (at >= L.Ap / 16) break;
#pragma unroll
        for (int i = 0; i < 6; ++i) w3[at][i] = wld(rs, L.wsp, (REFIL_WSP_W3 + at) * 6 + i, lane);
        b3q[at] = bld(rs, L.b3, at, lane);
    }
#pragma unroll
    for (int at = 0; at < 2; ++at) {
        if (at >= L.Ap / 16) break;
        const bf16x8(&w)[6] = w3[at];
        const floatx4 b3 = b3q[at];
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            floatx4 q = b3;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
                Split3 a3;
                a3.p[0] = w[kk * 3];
                a3.p[1] = w[kk * 3 + 1];
                a3.p[2] = w[kk * 3 + 2];
                q = mfma_x6(a3, hs3[i][kk], q);
            }
            if ((dd[i] >> col) & 1u) q = floatx4{0.f, 0.f, 0.f, 0.f};  // entity_rnn_agent.py:61
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ac = at * 16 + 4 * g + r;
                if (ac >= a.A) continue;
                const float v = ((avm[i] >> ac) & 1u) ? q[r] : -INFINITY;
                if (amax_better(v, ac, as[i].bv, as[i].bi)) {
                    as[i].bv = v;
                    as[i].bi = ac;
                }
            }
        }
    }
    stp.mark(22);
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        int act = argmax_reduce(as[i]);
        const int e = 2 * (p0 + i) + re;
        if (g == 0 && rn < a.NA && S.status[e] != 2) {
            if (!test_mode && eps > 0.f) {
                const uint64_t key = mlg_env_key(seed, b0 + e);
                const uint64_t r1 = mlg_rng(key, mlg_ctr(S.ep[e], (uint32_t)t, MLG_PURPOSE_EPS, (uint32_t)rn));
                if (mlg_u01(r1) < eps) {
                    const uint64_t r2 = mlg_rng(key, mlg_ctr(S.ep[e], (uint32_t)t, MLG_PURPOSE_RAND, (uint32_t)rn));
                    const int na = __popc(avm[i]);
                    if (na == 0) {
                        act = 0;
                    } else {
                        const int k = (int)(((r2 >> 40) * (uint64_t)na) >> 24);
                        uint32_t m = avm[i];
                        for (int j = 0; j < k; ++j) m &= m - 1;
                        act = __ffs((int)m) - 1;
                    }
                }
            }
            S.pact[e][rn] = act;
            bt.actions[((int64_t)S.slot[e] * bt.T1 + t) * a.NA + rn] = act;
        }
    }
    stp.mark(23);
}

// one-hot action rows of the running envs at step t from S.pact, all 64 lanes: lane (row = lane & 31, half = lane >> 5)
// of every env's NA x A block writes the floats [half * 12, half * 12 + 12) of one row (A <= 24).
__device__ inline void r4_onehot(const R4Lds& S, const RoArgs& a, const MlgEntityBatch& bt, int t, int lane) {
    const int row = lane & 31, half = lane >> 5;
    const int e = row >> 3, rn = row & 7;
    if (rn >= a.NA || S.status[e] == 2) return;
    const int act = S.pact[e][rn];
    float* oh = bt.actions_onehot + (((int64_t)S.slot[e] * bt.T1 + t) * a.NA + rn) * a.A;
    const int k0 = half * 12, k1 = min(a.A, k0 + 12);
    if (bt.full_write) {
        for (int k = k0; k < k1; ++k) oh[k] = k == act ? 1.f : 0.f;
    } else if (act >= k0 && act < k1) {
        oh[act] = 1.f;
    }
}

// SU > 0: the static shape of an SU-unit plan (refil_8: SU = 16, 8 agents, ED = 8, A = 5 + SU, last-action
// inputs): the agent layout offsets and the env dims become immediates instead of kernel-argument values held in
// SGPRs across the episode loop (as v7's static 5v5 / 3v3 shapes; SGPR spills 339 -> 222). Same code otherwise.
template <int KC1, int SU = 0>
__global__ void __launch_bounds__(64 * R4_WAVES) refil_rollout4_kernel(MlgEntityEnvSpec spec, MlgEnvState st,
                                                                       RAgent L_arg, const float* __restrict__ P,
                                                                       MlgEntityBatch bt, MlgRunInfo info, RoArgs a_arg,
                                                                       float eps, int test_mode) {
    const RAgent L = SU > 0 ? make_ragent(8 + MLG_ACT_BASE + SU, MLG_ACT_BASE + SU) : L_arg;
    RoArgs a = a_arg;
    if constexpr (SU > 0) {
        a.U = SU;
        a.NA = a.S = SU / 2;
        a.A = MLG_ACT_BASE + SU;
        a.ED = 8;
    }
    extern __shared__ __attribute__((aligned(16))) float ro_smem[];
    R4Shared& SH = *reinterpret_cast<R4Shared*>(ro_smem);
    const MlgEnvSpec& sp = spec.base;
    if (threadIdx.x < NE) {
        const int j = threadIdx.x;
        SH.team[j] = j < a.U ? sp.team[j] : 0;
        SH.role[j] = j < a.U ? sp.role[j] : 0;
        SH.melee[j] = j < a.U ? sp.melee[j] : 0;
        SH.agent[j] = j < a.NA ? j + 1 : 0;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    R4Lds& S = SH.S[wave];
    for (int i = lane; i < 2 * 16 * LDX; i += 64) (&S.o[0][0])[i] = 0.f;
    for (int i = lane; i < R4_ENVS * NE * 8; i += 64) (&S.feat[0][0][0])[i] = 0.f;
    __syncthreads();
    RStamps stp;
    stp.init();
    const int e = lane >> 4, u = lane & 15;  // env phase: lane = (env of the wave, unit)
    const int b0 = (blockIdx.x * R4_WAVES + wave) * R4_ENVS;
    if (lane < R4_ENVS) {
        const int b = b0 + lane;
        S.status[lane] = b < a.B ? 0 : 2;
        S.len[lane] = 0;
        S.ret[lane] = 0.f;
        S.stepped[lane] = 0;
        S.slot[lane] = b < a.B ? (int)ro_slot(bt, b) : 0;
        S.ep[lane] = b < a.B ? st.episode[b] : 0u;
    }
    if (lane < R4_ENVS * NAS) S.pact[lane >> 3][lane & 7] = 0;
    wave_sync();
    EnvTables T;
    T.team = SH.team;
    T.role = SH.role;
    T.melee = SH.melee;
    T.agent = SH.agent;
    T.U = a.U;
    T.grid = sp.grid;
    T.episode_limit = sp.episode_limit;
    T.stochastic = sp.stochastic;
    EnvMasks M0;
    M0.team1 = M0.healer = M0.tank = M0.melee = 0;
    for (int j = 0; j < a.U; ++j) {
        M0.team1 |= (uint32_t)(SH.team[j] != 0) << j;
        M0.healer |= (uint32_t)(SH.role[j] == 1) << j;
        M0.tank |= (uint32_t)(SH.role[j] == 0) << j;
        M0.melee |= (uint32_t)(SH.melee[j] != 0) << j;
    }
    M0.team1 = __builtin_amdgcn_readfirstlane(M0.team1);  // wave-uniform: scalar registers
    M0.healer = __builtin_amdgcn_readfirstlane(M0.healer);
    M0.tank = __builtin_amdgcn_readfirstlane(M0.tank);
    M0.melee = __builtin_amdgcn_readfirstlane(M0.melee);
    M0.U = a.U;
    M0.grid = sp.grid;
    // ---- reset (EnvWorker "reset", env_worker_process.py:54-60) ----
    const int b = b0 + e;
    const bool live = b < a.B;
    if (live && u < a.U) {
        const uint64_t key = mlg_env_key(sp.seed, b);
        const uint32_t ep = S.ep[e];
        const int k = entity_team_k(key, ep, a.kmin, a.kmax);
        const int tf = SH.team[u] ? a.S : 0;
        int xx, yy, hh;
        env_spawn_xyh(T, key, ep, u, tf, a.S, xx, yy, hh);
        if (u - tf >= k) hh = 0;
        S.x[e][u] = xx;
        S.y[e][u] = yy;
        S.hp[e][u] = hh;
        S.pk[e][u] = pk_pack(xx, yy, hh);
    }
    if (u >= a.U) S.pk[e][u] = 0;
    wave_sync();
    r4_observe(S, T, M0, a, bt, e, u, live, 0);
    wave_sync();
    floatx4 h0[4], h1[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) h0[i] = h1[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    uint64_t rows = 0;
    for (int t = 0;; ++t) {
        const int s0 = S.status[0], s1 = S.status[1], s2 = S.status[2], s3 = S.status[3];
        const bool p0 = s0 != 2 || s1 != 2, p1 = s2 != 2 || s3 != 2;
        if (!p0 && !p1) break;
        // opaque per-iteration copy of the weight pointer: keeps the compiler from hoisting the (loop-invariant)
        // weight loads of the step out of the episode loop into registers (the two-env kernel's LICM note)
        int64_t zoff = 0;
        asm volatile("" : "+s"(zoff));
        const float* __restrict__ Pw = P + zoff;
        rows += (uint64_t)a.NA * (uint64_t)((s0 != 2) + (s1 != 2) + (s2 != 2) + (s3 != 2));
        stp.mark(0);
        stp.step_begin();
        // ---- agent phase: EntityMAC.forward(t) + epsilon-greedy for the four envs ----
        // a pair with one env left runs only that env's entity tile
        if (s0 != 2 && s1 != 2) r4_entity_pair<KC1, 3>(Pw, L, S, 0, a, t, lane, stp);
        else if (s0 != 2) r4_entity_pair<KC1, 1>(Pw, L, S, 0, a, t, lane, stp);
        else if (s1 != 2) r4_entity_pair<KC1, 2>(Pw, L, S, 0, a, t, lane, stp);
        if (s2 != 2 && s3 != 2) r4_entity_pair<KC1, 3>(Pw, L, S, 1, a, t, lane, stp);
        else if (s2 != 2) r4_entity_pair<KC1, 1>(Pw, L, S, 1, a, t, lane, stp);
        else if (s3 != 2) r4_entity_pair<KC1, 2>(Pw, L, S, 1, a, t, lane, stp);
        stp.mark(1);
        // tile row r = env 2p + (r >> 3), agent r & 7; dead = agent entity masked or padding row >= n_agents
        const uint32_t pad = ~((1u << a.NA) - 1u) & 0xFFu;
        const uint32_t dead0 = ((S.em[0] & 0xFFu) | pad) | (((S.em[1] & 0xFFu) | pad) << 8);
        const uint32_t dead1 = ((S.em[2] & 0xFFu) | pad) | (((S.em[3] & 0xFFu) | pad) << 8);
        if (p0 && p1) {
            r4_post<2>(Pw, L, S.o[0], S.o[1], dead0, dead1, h0, h1, lane, stp);
        } else if (p0) {
            r4_post<1>(Pw, L, S.o[0], nullptr, dead0, 0u, h0, h1, lane, stp);
        } else {
            r4_post<1>(Pw, L, S.o[1], nullptr, dead1, 0u, h1, h0, lane, stp);
        }
        stp.mark(2);
        if (p0 && p1) {
            r4_select<2>(Pw, L, S, a, bt, sp.seed, b0, 0, dead0, dead1, h0, h1, eps, test_mode, t, lane, stp);
        } else if (p0) {
            r4_select<1>(Pw, L, S, a, bt, sp.seed, b0, 0, dead0, 0u, h0, h1, eps, test_mode, t, lane, stp);
        } else {
            r4_select<1>(Pw, L, S, a, bt, sp.seed, b0, 1, dead1, 0u, h1, h0, eps, test_mode, t, lane, stp);
        }
        wave_sync();
        r4_onehot(S, a, bt, t, lane);
        stp.mark(3);
        // ---- env phase (EnvWorker "step", env_worker_process.py:32-53), lane = (env, unit) ----
        // the unit tables as per-step opaque copies: the unrolled unit scans derive ~16 uniform bits per table, which
        // the compiler otherwise hoists out of the episode loop and spills (v_readlane reloads every step)
        EnvMasks M = M0;
        asm volatile("" : "+s"(M.team1), "+s"(M.healer), "+s"(M.tank), "+s"(M.melee));
        const bool stepping = S.status[e] == 0;
        int pk[16];
        load16(S.pk[e], pk);
        const int pu = S.pk[e][u];
        {  // executed action: validated policy action or scripted AI (spec §3.4)
            uint32_t tb, kb, ka, ke;
            unit_scan<16>(M, pk, u, pu, false, tb, kb, ka, ke);
            if (stepping && u < a.U) {
                int ac;
                if (u < a.NA) {
                    const int pa = S.pact[e][u];
                    const uint32_t av = pkh(pu) <= 0 ? 1u
                                                     : (((uint32_t)(pky(pu) + 1 < M.grid) << 1) |
                                                        ((uint32_t)(pky(pu) - 1 >= 0) << 2) |
                                                        ((uint32_t)(pkx(pu) + 1 < M.grid) << 3) |
                                                        ((uint32_t)(pkx(pu) - 1 >= 0) << 4) | (tb << MLG_ACT_BASE));
                    ac = (pa >= 0 && pa < MLG_ACT_BASE + a.U && ((av >> pa) & 1u)) ? pa : 0;
                } else {
                    ac = ai_from_scan(M, u, pu, kb, ka, ke, [&](int j) { return S.pk[e][j]; });
                }
                S.act[e][u] = ac;
            }
        }
        wave_sync();
        stp.mark(4);
        if (stepping && u < a.U) {
            int acts[16];
            load16(S.act[e], acts);
            S.nhp[e][u] = resolve_hp_reg(M, pk, acts, u, pu);
        }
        wave_sync();
        stp.mark(5);
        if (stepping && u < a.U && S.hp[e][u] > 0) env_apply_move(S.act[e][u], &S.x[e][u], &S.y[e][u]);
        // per-unit step results as lane ballots (bit 16 e + u): alive after, killed, bits of the hp lost (<= 64)
        uint64_t rw_alive, rw_kill, rw_loss[7];
        {
            const bool v = stepping && u < a.U;
            const int hb0 = v ? S.hp[e][u] : 0, hb1 = v ? S.nhp[e][u] : 0;
            const int loss = (hb0 > 0 && hb0 > hb1) ? hb0 - hb1 : 0;
            rw_alive = __ballot(v && hb1 > 0);
            rw_kill = __ballot(v && hb0 > 0 && hb1 == 0);
#pragma unroll
            for (int bb = 0; bb < 7; ++bb) rw_loss[bb] = __ballot((loss >> bb) & 1);
        }
        if (u == 0) {
            const int stt = S.status[e];
            S.stepped[e] = 0;
            const int64_t sl = (int64_t)S.slot[e] * bt.T1 + t;
            if (stt == 1) {  // final action recorded (parallel_stepper.py:153); env done
                S.status[e] = 2;
                if (bt.full_write) {
                    bt.reward[sl] = 0.f;
                    bt.terminated[sl] = 0;
                }
            } else if (stt == 0) {
                int alive[2], lost[2] = {0, 0}, kills[2];
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
                (void)kills[1];
                const int done = alive[0] == 0 || alive[1] == 0 || t + 1 >= sp.episode_limit;
                const int w0 = alive[1] == 0 && alive[0] > 0, w1 = alive[0] == 0 && alive[1] > 0;
                const float r = (float)(lost[1] + 10 * kills[0] + 200 * w0) * 0.0625f;  // policy team 0
                bt.reward[sl] = r;
                bt.terminated[sl] = (uint8_t)done;
                S.ret[e] += r;
                S.stepped[e] = 1;
                if (done) {
                    S.status[e] = 1;
                    S.len[e] = t + 1;
                    info.won[2 * b] = w0;
                    info.won[2 * b + 1] = w1;
                    info.draw[b] = !w0 && !w1;
                }
            }
        }
        wave_sync();
        stp.mark(6);
        const bool stepped = S.stepped[e] != 0;
        if (stepped && u < a.U) {
            S.hp[e][u] = S.nhp[e][u];
            S.pk[e][u] = pk_pack(S.x[e][u], S.y[e][u], S.nhp[e][u]);
        }
        wave_sync();
        r4_observe(S, T, M, a, bt, e, u, stepped, t + 1);
        wave_sync();
        stp.mark(7);
        stp.step_end(p0 && p1 ? 0 : 1);
    }
    // ---- finish: run summary, env state, full-write tails ----
    if (live && u == 0) {
        info.ep_len[b] = S.len[e];
        info.ret[b] = S.ret[e];
        st.t[b] = S.len[e];
        st.episode[b] = S.ep[e] + 1u;
    }
    if (live && u < a.U) {
        st.x[(int64_t)b * a.U + u] = S.x[e][u];
        st.y[(int64_t)b * a.U + u] = S.y[e][u];
        st.hp[(int64_t)b * a.U + u] = S.hp[e][u];
    }
    if (bt.full_write) {
        for (int ee = 0; ee < R4_ENVS; ++ee)
            if (b0 + ee < a.B) ro_zero_tail(bt, a, S.slot[ee], S.len[ee] + 1, lane);
    }
    if (info.agent_rows && lane == 0) atomicAdd((unsigned long long*)info.agent_rows, (unsigned long long)rows);
    stp.mark(8);
    stp.flush();
}
