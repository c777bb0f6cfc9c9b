// rollout_sp8_mix.inc -- sp8 against an opponent mixture (sp8-mix; included by rollout.hip after rollout_sp8.inc).
//
// mlg_rollout_selfplay_mix for the shapes sp8 serves: an sp8 workgroup plays RS8 = 16 envs, which is one group of
// the mixture, so workgroup g reads its away policy from the packed pool by groups[g].away (a wave-uniform pointer
// where rollout_sp8_kernel has its P1 argument) and its roster tables from specs[groups[g].spec] in device memory
// (sp8_prologue -> load_spec_tables; every later phase reads the tables from LDS). The scalars of the env (U, grid,
// episode limit, seed, ...) are the same in every spec of a launch and travel as the spec0 kernel argument.
//
// The step loop is rollout_sp8_kernel's, written out again: a second kernel, not a template flag or a shared body, so
// that the code of the existing <10, 10> / <6, 6> instantiations stays what it was (their resource usage is compared
// against the parent's in profiles/league_mix/resource_usage.txt). The phase functions (sp8_fc1, sp8_gru_side,
// sp8_fc2, the env lanes) are shared: they take the weight pointers as arguments. Env b's arithmetic does not depend
// on the other envs of its workgroup (a row of an MFMA tile depends on its own inputs only), so its rows are
// bit-identical to the plain sp8 launch with that one (away, spec).

struct SP8Mix {
    const float* pool;
    int64_t pool_stride;  // floats per packed policy
    const MlgMixGroup* groups;
    const MlgEnvSpec* specs;
    int n_pool, n_specs;
};

template <int SN, int SU>
__global__ void __launch_bounds__(512, 2) rollout_sp8_mix_kernel(MlgEnvSpec spec, MlgEnvState st,
                                                                const float* __restrict__ P0, SP8Mix mix,
                                                                MlgBatch bt0_arg, MlgBatch bt1_arg, MlgRunInfo info,
                                                                float eps0, float eps1, int test_mode) {
    using S = StaticShapeSP8<SN, SU>;
    const AgentLayout& L = S::L;
    const RolloutLdsSP8& lay = S::lay;
    constexpr int NT = SN, nh = SN / 2, NW = 8, TS = (RS8 * nh + 15) / 16, KK = (S::L.Dob + 31) / 32;
    const MlgBatch bt0 = split_batch_sgprs(bt0_arg), bt1 = split_batch_sgprs(bt1_arg);
    extern __shared__ __attribute__((aligned(16))) int smem[];
    float* fm = reinterpret_cast<float*>(smem);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), hl = lane & 31;
    const int e0 = blockIdx.x * RS8, T1 = bt0.T1;
    // The host validated its copy of the group table; the launch reads the caller's device copy. A device row that is
    // out of range plays nothing instead of reading past the pool or the spec array.
    const MlgMixGroup grp = mix.groups[blockIdx.x];
    if ((unsigned)grp.away >= (unsigned)mix.n_pool || (unsigned)grp.spec >= (unsigned)mix.n_specs) {
        const int b = e0 + (int)threadIdx.x;
        if (threadIdx.x < RS8 && b < bt0.B) {
            info.ep_len[b] = -1;
            info.ret[b] = 0.f;
            if (info.ret_away) info.ret_away[b] = 0.f;
            info.won[2 * b] = info.won[2 * b + 1] = 0;
            info.draw[b] = 0;
        }
        return;
    }
    const float* __restrict__ P1 = mix.pool + (int64_t)grp.away * mix.pool_stride;
    sp8_prologue(mix.specs[grp.spec], L, P0, P1, lay, smem);  // the group's roster, from device memory
    EnvCtxSP C;
    {
        RolloutLds2 l2{};  // EnvCtx view of the env / table carve (same field names)
        l2.env = lay.env;
        l2.pk = lay.pk;
        l2.act = lay.act;
        l2.am = lay.am;
        l2.obs = lay.reg;  // obs rows of step 0: region 0
        l2.avail = lay.avail;
        l2.ldo = lay.ldo;
        l2.xpl = 1;  // bf16 obs rows (EnvCtx::obf)
        static_cast<EnvCtx&>(C) = make_env_ctx(spec, l2, smem, bt0, info, SU, NT, 5 + SU, true);
    }
    C.bt2 = bt1;
    C.nh = nh;
    EnvLaneSP E;
    sp_lane_reset<false, RS8>(C, st, E, wave * 2 + (lane >> 5), e0, hl);
    const int side = wave >> 2, fb = wave & 3;  // fc1: side and output chunk of this wave
    GruG8 W8;
    int wside = 0;  // side whose GRU weights W8 holds (sp7's swap scheme)
    load_gru_gsp(W8, P0, L, lay.sw[0].gb, wave, lane);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)  // consumed before the loop (see load_gru_chunk)
#pragma unroll
        for (int q = 0; q < 3; ++q)
            asm volatile("" : "+v"(W8.rzi[kk].p[q]), "+v"(W8.rzh[kk].p[q]), "+v"(W8.n[kk].p[q]));
    // this lane's two GRU output features after the permlane exchange (as ph_gru_g8)
    const int fo = 8 * wave + 4 * ((lane >> 4) & 1) + (lane >= 32 ? 2 : 0);
    __syncthreads();
    const uint32_t wm = (1u << nh) - 1u;
    int* wmap = smem + lay.rmap + wave * lay.rms;
    uint32_t m_prev = 0u;
    int x_prev = 0;
    uint64_t rows_issued = 0;
    Stamps sp;  // diagnostic build only: the slots of rollout_sp8_kernel
    sp.init();
    for (int t = 0; t < T1; ++t) {
        const uint32_t run = (uint32_t)__ballot(lane < RS8 && C.R.status[lane & (RS8 - 1)] < 2);
        sp.step(t, __popc(run));
        if (run == 0) break;
        make_rmap_sp8<TS>(C.amask, wmap, nh, wm, lane, m_prev, x_prev);
        sp.mark(14);
        rows_issued += 2 * TS * 16;
        float* Rc = fm + lay.reg + (t & 1) * lay.rsz;
        float* Rp = fm + lay.reg + ((t & 1) ^ 1) * lay.rsz;
        const int wrow = (lane & 15), wcol = (16 * fb + 4 * (lane >> 4)) / 2;  // this lane's plane row / word
        floatx4 acc[TS];
        sp8_fc1<KK, TS>(L, lay, fm, Rc, wmap, C.R.prev, side ? P1 : P0, side, fb, nh, NT, t, lane, acc);
        sp.mark(0);
        lds_barrier();  // every obs row of Rc read: x_t may overwrite them
        sp.mark(1);
#pragma unroll
        for (int u = 0; u < TS; ++u) sp8_store_planes(Rc + ((side * TS + u) * 16 + wrow) * XPL_STRIDE, wcol, acc[u]);
        const int sa = wside;
        sp.mark(2);
        lds_barrier();
        sp.mark(3);
        int pre = -1;  // epsilon coin of the wave's fc2 tile (global agent index: the map's field), off the fc2 path
        if (wave < 2 * TS) pre = eps_coin(spec, C.R, wmap, wave, e0, t, wave >= TS ? eps1 : eps0, test_mode, lane);
        float2 hA[TS], hB[TS];  // h' of the side W8 holds on entry (A), then of the other side (B)
        {
            int zero = 0;  // opaque offset: both sides' loads must not be hoisted out of the step loop
            asm volatile("" : "+s"(zero));
            const float* Pn = (sa ? P0 : P1) + zero + L.gsp;
            // the other side's weights are requested per K step inside the last tile of side A (split swap)
            sp8_gru_side<TS, true>(W8, fm, Rc, Rp, wmap, sa, fo, lane, hA, Pn, wave);
            const int gbn = sa ? lay.sw[0].gb : lay.sw[1].gb, H = 64, gg = lane >> 4, fo8 = 8 * wave + 4 * (gg & 1);
            W8.rz_bias = gbn + (gg < 2 ? fo8 : H + fo8);  // as load_gru_gsp
            W8.in_bias = gbn + 2 * H + fo8;
            W8.hn_bias = gbn + 3 * H + fo8;
            wside = 1 - sa;
        }
        sp8_gru_side<TS>(W8, fm, Rc, Rp, wmap, 1 - sa, fo, lane, hB);
        sp.mark(4);
        lds_barrier();  // x_t and h_{t-1} read by every wave: h'_t may overwrite x_t
        sp.mark(5);
#pragma unroll
        for (int u = 0; u < TS; ++u) {
            const int ca = (sa * TS + u) * 16 + wrow, cb = ((1 - sa) * TS + u) * 16 + wrow;
            if (wmap[ca] & 1) sp8_store_planes2(Rc + ca * XPL_STRIDE, fo / 2, hA[u]);
            if (wmap[cb] & 1) sp8_store_planes2(Rc + cb * XPL_STRIDE, fo / 2, hB[u]);
        }
        sp.mark(6);
        lds_barrier();
        sp.mark(7);
        sp8_fc2(spec, L, lay, fm, Rc, wmap, C.R, bt0, bt1, P0, P1, TS, 2 * TS, wave, NW, e0, t, eps0, eps1, test_mode,
                lane, pre);
        sp.mark(8);
        lds_barrier();
        sp.mark(9);
        EnvCtxSP Ce = sp_ctx_step(C);
        Ce.lobs = Rp;  // observation rows of t + 1 into the region h_{t-1} held (read by the GRU above)
        sp_lane_step1<false>(Ce, E, t, hl);
        sp.mark(10);
        sp_lane_step2<false>(Ce, E, t, hl);
        if (E.stepped) sp8_obs_pad(Ce, E.e, hl);
        sp.mark(11);
        if (!E.stepped && (t & 1)) sp_lane_tail<false>(Ce, E, 8, hl);
        sp.mark(12);
        lds_barrier();
        sp.mark(13);
    }
    sp.flush();
    if (threadIdx.x == 0 && info.agent_rows) atomicAdd(info.agent_rows, (unsigned long long)rows_issued);
    sp_lane_finish<false>(C, st, E, hl);
}
