// learner.hip -- QLearner.train (src/marl/learners/q_learner.py:34-131) as one device pipeline on gfx950.
//
//   pack        online/target agent + mixer weights -> kernel layouts (+ W_ih^T for backward)
//   mask_sum    mask = filled[:, :-1] * (1 - terminated shifted) and its sum                (:36-42, :89-98)
//   agent_in    fc1 + W_ih x for every (t, row), online + target, fully parallel               (:44-65)
//   agent_rec4  the recurrence only (W_hh h + gates), one workgroup per 4 sequence rows,
//               wave w owns hidden chunk w with its W_hh rows in VGPRs; saves gates
//   agent_q     fc2 for every (t, row), fully parallel
//   mix_td      per (b, t) row: gather chosen Q, double-Q target, QMixer fwd (online+target),
//               TD error, masked MSE partials, QMixer backward -> dQ and mixer deltas         (:55-98)
//   per_reduce  prioritized replay only (cfg.per = 1): the per-episode errors from the TD kernel's rows
//   agent_bwd4  reverse-time GRU backward on 4-row tiles (gru4_device.h)                     (:103)
//   agent_dx    dX = W_ih^T dGI * relu' for every (t, row), fully parallel
//   wgrad       every weight/bias gradient as sum_rows delta^T x, one wave per 64x64 block and row chunk
//               (deterministic slab reduction; MFMA with the row index as K)
//   finish      loss/stat reduction, clip_grad_norm_(10), RMSprop step                       (:104-105, learner.py:25-31)
// Work whose result nothing reads is not run (Skip, below): steps past the episodes of a 16-row tile, (b, t) mixer
// rows past the episode's last unmasked transition, and the whole target pass while the target parameters are a
// bit copy of the online ones. MLG_LEARNER_FULL=1 (read per call) runs every row to max_t_filled and both nets.
// Tensors saved for backward are t-major: [T][R][F] with R = B * N agent rows (r = b * N + n).
// MlgLearnerCfg.distinct = 1 (one DRQN per agent slot): the agent kernels' <H, true> forms run N instances of the
// N = 1, R = B problem by a grid coordinate (Distinct networks, below); the mixer side is unchanged.
//
// Mixers (MlgLearnerCfg.mixer / hypernet_layers; everything else is refused by check_cfg):
//   0 none (IQL)   iql_td: td[b,t,n] = Q_chosen[b,t,n] - (r[b,t] + gamma (1 - term[b,t]) target[b,t+1,n]), the target
//                  per agent as for VDN/QMIX. The reference expands the mask over the agents (q_learner.py:89-98), so
//                  every denominator is mask_elems = N sum(mask): loss = sum(mask td^2) / mask_elems, td_error_abs
//                  likewise; q_taken_mean and target_mean divide by mask_elems * N (the reference's double division,
//                  kept). stats[5] = mask_elems, stats[6] = count_nonzero of the expanded mask = N count_nonzero(mask),
//                  which is also what trained_steps grows by. n_mixer = 0: no mixer pack, no mixer jobs.
//   1 vdn          mix_td (sum over agents)
//   2 qmix         hypernet_layers 2: mixing_embed_dim E in {16, 32, 64}, hypernet_embed HE in {32, 64, 128}. E = 32,
//                  HE = 64 keeps its prefetching / split forms (MixerPF, rec4_mixpre + mix_td2); the other widths run
//                  the generic one-kernel mix_td<HE, E>.
//                  hypernet_layers 1 (qmix.py:17, the reference's fallback): hyper_w_1 = Linear(S, N E) and
//                  hyper_w_final = Linear(S, E) read the state directly; mix_td1<E>, E in {16, 32, 64}. Flat order
//                  hyper_w_1.{weight, bias}, hyper_w_final.{weight, bias}, hyper_b_1.{weight, bias},
//                  V.{0.weight, 0.bias, 2.weight, 2.bias}.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "agent_device.h"
#include "agent_ff_device.h"
#include "batch_mask_device.h"
#include "gru4_device.h"
#include "mlg_host.h"
#include "wgrad_device.h"

namespace {

using WJobs = mlg::BJobsT<16>;
using mlg::block_sum_1024;

// ---- canonical flat parameter offsets (nn.Module named_parameters order) ------------------------
struct AgentOffs {
    int64_t fc1w, fc1b, wih, whh, bih, bhh, fc2w, fc2b, total;
};
__host__ __device__ inline AgentOffs agent_offs(int H, int d_in, int A) {
    AgentOffs o;
    int64_t p = 0;
    o.fc1w = p; p += (int64_t)H * d_in;
    o.fc1b = p; p += H;
    o.wih = p; p += (int64_t)3 * H * H;
    o.whh = p; p += (int64_t)3 * H * H;
    o.bih = p; p += 3 * H;
    o.bhh = p; p += 3 * H;
    o.fc2w = p; p += (int64_t)A * H;
    o.fc2b = p; p += A;
    o.total = p;
    return o;
}

// Feed-forward agent (MlgLearnerCfg.agent = 1): fc1.weight, fc1.bias, fc2.weight, fc2.bias; the GRU entries are empty.
__host__ __device__ inline AgentOffs ff_offs(int H, int d_in, int A) {
    AgentOffs o;
    int64_t p = 0;
    o.fc1w = p; p += (int64_t)H * d_in;
    o.fc1b = p; p += H;
    o.wih = o.whh = o.bih = o.bhh = p;
    o.fc2w = p; p += (int64_t)A * H;
    o.fc2b = p; p += A;
    o.total = p;
    return o;
}

struct MixOffs {
    int64_t w1_0w, w1_0b, w1_2w, w1_2b, wf_0w, wf_0b, wf_2w, wf_2b, b1w, b1b, v0w, v0b, v2w, v2b, total;
};
// One layer: w1_0 / wf_0 are hyper_w_1 [N E][S] and hyper_w_final [E][S] themselves; the .2 entries are empty.
__host__ __device__ inline MixOffs mix_offs(int N, int S, int E, int HE, int layers) {
    MixOffs o;
    int64_t p = 0;
    const bool two = layers != 1;
    const int64_t r0 = two ? HE : (int64_t)N * E, r1 = two ? HE : E;
    o.w1_0w = p; p += r0 * S;
    o.w1_0b = p; p += r0;
    o.w1_2w = p; p += two ? (int64_t)N * E * HE : 0;
    o.w1_2b = p; p += two ? (int64_t)N * E : 0;
    o.wf_0w = p; p += r1 * S;
    o.wf_0b = p; p += r1;
    o.wf_2w = p; p += two ? (int64_t)E * HE : 0;
    o.wf_2b = p; p += two ? E : 0;
    o.b1w = p; p += (int64_t)E * S;
    o.b1b = p; p += E;
    o.v0w = p; p += (int64_t)E * S;
    o.v0b = p; p += E;
    o.v2w = p; p += E;
    o.v2b = p; p += 1;
    o.total = p;
    return o;
}

// ---- packed mixer block: m1 = [w1h | wfh | b1 | vh] rows over padded state, transposes, padded V.2 ----
// One layer: the rows that read the state are m1 = [hyper_w_1 (N E rows) | hyper_w_final | b1 | vh]; a2T and f2T are
// empty. r0 / r1 = rows of m1's first two blocks (HE, HE or N E, E).
struct MixPack {
    int L1, Sp, NE, r0, r1;
    int64_t m1, mb1, a2T, f2T, v2p, bv2p, total;
};
__host__ __device__ inline MixPack mix_pack(int N, int S, int E, int HE, int layers) {
    MixPack m;
    const bool two = layers != 1;
    m.NE = N * E;
    m.r0 = two ? HE : m.NE;
    m.r1 = two ? HE : E;
    m.L1 = m.r0 + m.r1 + 2 * E;
    m.Sp = (S + 15) / 16 * 16;
    int64_t p = 0;
    m.m1 = p; p += (int64_t)m.L1 * m.Sp;
    m.mb1 = p; p += m.L1;
    m.a2T = p; p += two ? (int64_t)HE * m.NE : 0;
    m.f2T = p; p += two ? (int64_t)HE * E : 0;
    m.v2p = p; p += (int64_t)16 * E;
    m.bv2p = p; p += 16;
    m.total = mlg_align4(p);
    return m;
}

struct MixPtrs {
    const float *m1, *mb1, *a2, *ba2, *a2T, *f2, *bf2, *f2T, *v2p, *bv2p;
};

// ---- device config ---------------------------------------------------------------------------------
struct LCfg {
    int B, T, T1, N, A, Ap, d_obs, d_in, H, S, E, HE, mixer, double_q, last_action, agent_id;
    int R, RM;
    float gamma;
    int full;  // MLG_LEARNER_FULL: no skipping
    int ff;    // MlgLearnerCfg.agent = 1: the feed-forward agent (no recurrence kernels, no GRU buffers)
    int dx;    // MlgLearnerCfg.distinct = 1: one network per agent slot (Distinct networks, below)
};

// ---- Distinct networks (cfg.distinct = 1) ---------------------------------------------------------
// The agent part of a call is N instances of the shared-agent problem with N = 1 and R = B rows: instance `ag` (a grid
// coordinate of every agent kernel's <H, true> form) runs network ag on the rows of agent slot ag. Its packed weights,
// W_ih^T and every agent-side workspace tensor ([T][B][F], rows r = b) lie at ag times a per-agent stride, all
// multiples of four floats; the Skip tables and the agent row bitmap are those of one instance (l16 per tile of 16
// episodes) and shared by all. The mixer side keeps its layout, rows r = b N + n: the instances meet it where they
// read the batch (obs / last action of slot ag), where agent_q stores Q into mac / tmac, and where the reverse
// recurrence and fc2's weight-gradient job read dq / d2 (row stride N). The mixer and TD kernels run unchanged.
struct DxView {
    int ag;                                  // network = agent slot
    int64_t p, in, h, hs, g3;                // float offsets of instance ag: packed block, [T][B][d_in], [T][B][H],
                                             // [T + 1][B][H], [T][B][3H] (agent_dx_kernel, which has no layout
                                             // argument, forms its own: W_ih^T blocks are 3 H H apart)
};
__host__ __device__ inline int64_t dx_in_stride(const LCfg& c) { return mlg_align4((int64_t)c.T * c.B * c.d_in); }
__device__ __forceinline__ DxView dx_view(const LCfg& c, const AgentLayout& L, int ag) {
    const int64_t TB = (int64_t)c.T * c.B;
    return DxView{ag, (int64_t)ag * L.gsp, ag * dx_in_stride(c), ag * TB * c.H, ag * (TB + c.B) * c.H, ag * TB * 3 * c.H};
}

// What a call skips, from prep_kernel (workspace; every kernel after it reads the same three):
//   mlen[b]   1 + the last t < t_eff - 1 with mask(b, t) != 0: transition (b, t) is live iff t < mlen[b]; the dead
//             ones have mask 0, so every delta of theirs is an exact zero
//   l16[tile] steps the agent kernels run for the rows 16 tile .. 16 tile + 15: clamp(max mlen[b] + 1, 2, t_eff)
//             (the target of transition t reads step t + 1); block (tile, t) is live iff t < l16[tile]. The
//             recurrences' 4-row tiles run their 16-row tile's steps, so a live block is whole: no kernel reads a
//             workspace row this call did not write. Exact integers in float.
//   abits, mbits  the same two predicates per row of the weight-gradient jobs, as bitmaps (wgrad_device.h
//             bjob_row_bits): agent row t R + r live iff t < l16[r / 16], mixer row b (T - 1) + t iff t < mlen[b]
//   flag      1 iff some target parameter differs bitwise from its online parameter (stored by prep_kernel's blocks,
//             cleared by finish_kernel). Otherwise the target network's blocks return at once and its consumers read
//             the online buffers, which hold the same bits.
// full: mlen = t_eff - 1 and l16 = t_eff everywhere, target pass always.
struct Skip {
    const float *mlen, *l16;
    const unsigned* flag;
};
__device__ __forceinline__ bool target_runs(const LCfg& c, const Skip& k) { return c.full || *k.flag == 1u; }
__device__ __forceinline__ int tile_steps(const Skip& k, int tile) { return (int)k.l16[tile]; }

// ---- workspace layout --------------------------------------------------------------------------------
struct WsLayout {
    int64_t p_on, p_tg, wihT, mix_on, mix_tg;
    int64_t in, x, hs, hs_tg, gi_on, gi_tg, gr, gz, gn, ghn, mac, tmac, dq, d2, dgi, dgh, da;
    int64_t srow, l1act, d1, da2, df2, dv2, hyp_on, hyp_tg;
    int64_t part, msum, rows, mlen, l16, flag, alive, abits, mbits, tdrow, nrm, slab, total;
    int n_mix_tiles, n_tasks, hyp_stride;
};

__host__ __device__ inline int64_t a4(int64_t v) { return mlg_align4(v); }

// ================================================================================================
// packing
__device__ __forceinline__ float pack_mixer_elem(const MixPack& mp, const MixOffs& mo, const float* __restrict__ P,
                                                 int64_t i, int S, int E, int HE) {
    float v = 0.f;
    const int r0 = mp.r0, r01 = mp.r0 + mp.r1;  // HE, 2 HE (one layer: N E, N E + E)
    if (i < mp.mb1) {
        const int r = (int)(i / mp.Sp), c = (int)(i % mp.Sp);
        if (c < S) {
            if (r < r0) v = P[mo.w1_0w + (int64_t)r * S + c];
            else if (r < r01) v = P[mo.wf_0w + (int64_t)(r - r0) * S + c];
            else if (r < r01 + E) v = P[mo.b1w + (int64_t)(r - r01) * S + c];
            else v = P[mo.v0w + (int64_t)(r - r01 - E) * S + c];
        }
    } else if (i < mp.a2T) {
        const int r = (int)(i - mp.mb1);
        if (r < r0) v = P[mo.w1_0b + r];
        else if (r < r01) v = P[mo.wf_0b + r - r0];
        else if (r < r01 + E) v = P[mo.b1b + r - r01];
        else v = P[mo.v0b + r - r01 - E];
    } else if (i < mp.f2T) {  // a2T [HE][NE] = w1_2w^T (two layers only)
        const int64_t k = i - mp.a2T;
        const int r = (int)(k / mp.NE), c = (int)(k % mp.NE);
        v = P[mo.w1_2w + (int64_t)c * HE + r];
    } else if (i < mp.v2p) {  // f2T [HE][E]
        const int64_t k = i - mp.f2T;
        const int r = (int)(k / E), c = (int)(k % E);
        v = P[mo.wf_2w + (int64_t)c * HE + r];
    } else if (i < mp.bv2p) {  // v2p [16][E], row 0 = V.2.weight
        const int64_t k = i - mp.v2p;
        if (k < E) v = P[mo.v2w + k];
    } else if (i < mp.bv2p + 16) {
        if (i == mp.bv2p) v = P[mo.v2b];
    }
    return v;
}

// episode b of the batch -> its slot in the tensors (sampled view of the replay buffer: rows[b])
__device__ __forceinline__ int64_t bslot(const MlgBatch& bt, int b) { return bt.rows ? (int64_t)bt.rows[b] : (int64_t)b; }

// ================================================================================================
// mask: mask[b][t] = filled[b][t] * (t > 0 ? 1 - terminated[b][t-1] : 1), t < T-1
__device__ __forceinline__ float mask_at(const MlgBatch& bt, int b, int t) {
    const int64_t base = bslot(bt, b) * bt.T1;
    float m = (float)bt.filled[base + t];
    if (t > 0) m *= 1.f - (float)bt.terminated[base + t - 1];
    return m;
}

// Fused learner prologue (one launch instead of eight): block 0 sums the mask (batch_mask_device.h); the other blocks
// pack the online / target agent weights (pack_agent_elem), transpose W_ih (dX pass), pack the online / target
// QMixer hypernets (pack_mixer_elem), zero the sparse delta buffers d2 and dq and compare the target parameters with
// the online ones (Skip::flag). The target packs always run: whether they are needed is known only after this launch.
struct PrepJob {
    AgentLayout L;
    MlgAgentParams ap_on, ap_tg;
    float *p_on, *p_tg;
    const float* wih;  // [3H][H] -> wihT [H][3H]
    float* wihT;
    int rows3, cols;
    MixPack mp;
    MixOffs mo;
    const float *mix_src_on, *mix_src_tg;
    float *mix_on, *mix_tg;
    int N, S, E, HE, mixer;
    float *d2, *dq;
    int64_t n_d2, n_dq;
    MlgBatch bt;
    int B, T;
    float* msum;
    float *mlen, *l16;      // Skip tables, written by block 0 after the mask statistics
    uint32_t *abits, *mbits;
    unsigned* flag;         // Skip::flag
    const float *cmp_on, *cmp_tg;  // the flat parameter vectors, compared bitwise
    int64_t n_cmp;
    int cmp_vec;            // both 16-byte aligned
    int R, full;
    int ff;                 // pack the feed-forward block (agent_ff_device.h) instead of the DRQN block
    int n_rows_in;          // > 0: the slot map travels here (host_rows); block 0 stores it to rows_dst
    int32_t* rows_dst;
    int32_t rows_in[MLG_INLINE_ROWS];
    // distinct networks (prep_kernel<true>): nag networks of ao_total flat floats each, packed at strides of L.gsp
    // (W_ih^T: 3 H H); R = B and N = 1 above (the tables of one instance); blocks 1 .. nag store alive[ag]
    int nag, nslots, A;     // nslots = the batch's agents per episode
    int64_t ao_total;
    unsigned* alive;
};
static_assert(sizeof(PrepJob) <= 3072, "PrepJob must fit the kernel-argument segment");

__device__ __forceinline__ float prep_pack_agent(const PrepJob& J, const MlgAgentParams& ap, int64_t k) {
    if (J.ff) return pack_ff_elem(J.L, MlgFFParams{ap.fc1_w, ap.fc1_b, ap.fc2_w, ap.fc2_b}, k);
    return pack_agent_elem(J.L, ap, k);
}

__device__ __forceinline__ MlgAgentParams shift_agent(const MlgAgentParams& p, int64_t o) {
    return MlgAgentParams{p.fc1_w + o, p.fc1_b + o, p.w_ih + o, p.b_ih + o, p.w_hh + o, p.b_hh + o, p.fc2_w + o, p.fc2_b + o};
}

// DX: the distinct-network form. Dead-slot rule: slot ag is alive iff some stored step of the batch
// (filled != 0, t < T) offers it an action other than action 0; block 1 + ag scans the slot's avail rows and stores
// alive[ag] (every call, so the word needs no initial value). The weight-gradient reduce reads it.
template <bool DX>
__global__ void __launch_bounds__(1024) prep_kernel(PrepJob J) {
    if constexpr (DX) {
        if (blockIdx.x >= 1 && (int)blockIdx.x <= J.nag) {
            __shared__ int32_t arows[MLG_INLINE_ROWS];
            MlgBatch b2 = J.bt;
            if (J.n_rows_in > 0) {
                if (threadIdx.x < J.n_rows_in) arows[threadIdx.x] = J.rows_in[threadIdx.x];
                __syncthreads();
                b2.rows = arows;
            }
            const int ag = (int)blockIdx.x - 1;
            int any = 0;
            for (int i = threadIdx.x; i < J.B * J.T; i += blockDim.x) {
                const int b = i / J.T, t = i - b * J.T;
                const int64_t st = bslot(b2, b) * b2.T1 + t;
                if (b2.filled[st] == 0) continue;
                const int32_t* av = b2.avail + (st * J.nslots + ag) * J.A;
                for (int a = 1; a < J.A; ++a) any |= av[a] != 0;
            }
            any = __syncthreads_or(any);
            if (threadIdx.x == 0) J.alive[ag] = any ? 1u : 0u;
            return;
        }
    }
    if (blockIdx.x == 0) {
        __shared__ int32_t srows[MLG_INLINE_ROWS];
        __shared__ mlg::MaskStatsLds ms;
        MlgBatch b2 = J.bt;
        if (J.n_rows_in > 0) {  // the block reads the slot map from LDS; later launches from rows_dst
            if (threadIdx.x < J.n_rows_in) {
                srows[threadIdx.x] = J.rows_in[threadIdx.x];
                J.rows_dst[threadIdx.x] = J.rows_in[threadIdx.x];
            }
            __syncthreads();
            b2.rows = srows;
        }
        constexpr int EPW = 4;  // episodes per wave: 16 waves cover batches of up to 64 episodes
        // the Skip tables stay in LDS for the passes below (up to TABMAX episodes / tiles; global memory otherwise)
        constexpr int TABMAX = 256;
        __shared__ float smlen[TABMAX], sl16[TABMAX];
        const int ntiles = (J.R + 15) / 16;
        float* ml = J.B <= TABMAX ? smlen : J.mlen;
        float* lt = ntiles <= TABMAX ? sl16 : J.l16;
        mlg::batch_mask<EPW>(b2.filled, b2.terminated, b2.T1, [&](int b) { return bslot(b2, b); }, J.B, J.T, J.msum, ml,
                             ms);
        __syncthreads();  // ml and ms.te are stored
        const int Te = min(max(ms.te, 2), J.T);  // = msum[1]
        for (int b = threadIdx.x; b < J.B; b += blockDim.x) {
            if (J.full) ml[b] = (float)(Te - 1);
            if (ml != J.mlen) J.mlen[b] = ml[b];
        }
        if (J.full) __syncthreads();
        for (int tile = threadIdx.x; tile < ntiles; tile += blockDim.x) {
            int m = 0;  // the tile's rows cover episodes (16 tile) / N .. (16 tile + 15) / N
            const int b1 = (min(J.R, tile * 16 + 16) - 1) / J.N;
            for (int b = tile * 16 / J.N; b <= b1; ++b) m = max(m, (int)ml[b] + 1);
            const float v = (float)min(max(m, 2), Te);
            lt[tile] = v;
            if (lt != J.l16) J.l16[tile] = v;
        }
        __syncthreads();  // lt is stored
        // the weight-gradient jobs' row bitmaps, a 32-row word per thread, by runs of rows that share a table entry:
        // agent rows t R + r by 16-row tile (whole run live iff t < l16), mixer rows b (T - 1) + t by episode (the
        // run's first mlen[b] - t rows live)
        const int TR = J.T * J.R, Tm = J.T - 1, RM = J.B * Tm;
        const int na = (TR + 31) / 32, nm = J.mixer == 2 ? (RM + 31) / 32 : 0;
        for (int j = threadIdx.x; j < na + nm; j += blockDim.x) {
            const bool ag = j < na;
            const int row0 = 32 * (ag ? j : j - na), D = ag ? J.R : Tm, rows = ag ? TR : RM;
            int hi = row0 / D, lo = row0 - hi * D, k = 0;
            uint32_t m = 0;
            while (k < 32 && row0 + k < rows) {
                const int run = ag ? min(((lo >> 4) + 1) << 4, D) - lo : D - lo;
                const int n = min(run, min(32 - k, rows - row0 - k));
                const int live = ag ? (hi < (int)lt[lo >> 4] ? n : 0) : min(max((int)ml[hi] - lo, 0), n);
                if (live > 0) m |= (live >= 32 ? 0xFFFFFFFFu : (1u << live) - 1u) << k;
                k += n;
                lo += n;
                if (lo == D) {
                    lo = 0;
                    ++hi;
                }
            }
            (ag ? J.abits : J.mbits)[ag ? j : j - na] = m;
        }
        return;
    }
    const int64_t na = J.ff ? J.L.total : J.L.gsp,  // the learner reads no pre-split rollout sections (gsp, w1s)
                   nt = (int64_t)J.rows3 * J.cols, nm = J.mixer == 2 ? J.mp.total : 0;
    const int nag = DX ? J.nag : 1, first = DX ? 1 + J.nag : 1;  // DX: blocks 1 .. nag scan the slots (above)
    const int64_t total = 2 * na * nag + nt * nag + 2 * nm + J.n_d2 + J.n_dq + (J.n_cmp + 3) / 4;
    for (int64_t i = (int64_t)(blockIdx.x - first) * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)(gridDim.x - first) * blockDim.x) {
        int64_t k = i;
        if constexpr (DX) {  // network ag's blocks: element by element what the shared agent's block holds
            if (k < 2 * na * nag) {
                const bool on = k < na * nag;
                if (!on) k -= na * nag;
                const int ag = (int)(k / na);
                k -= ag * na;
                const MlgAgentParams ap = shift_agent(on ? J.ap_on : J.ap_tg, ag * J.ao_total);
                (on ? J.p_on : J.p_tg)[ag * na + k] = pack_agent_elem(J.L, ap, k);
                continue;
            }
            k -= 2 * na * nag;
            if (k < nt * nag) {
                const int ag = (int)(k / nt);
                k -= ag * nt;
                const int r = (int)(k / J.cols), c = (int)(k % J.cols);
                J.wihT[ag * nt + (int64_t)c * J.rows3 + r] = J.wih[ag * J.ao_total + k];
                continue;
            }
            k -= nt * nag;
        } else {
            if (k < na) { J.p_on[k] = prep_pack_agent(J, J.ap_on, k); continue; }
            k -= na;
            if (k < na) { J.p_tg[k] = prep_pack_agent(J, J.ap_tg, k); continue; }
            k -= na;
            if (k < nt) {  // wihT[c][r] = wih[r][c]
                const int r = (int)(k / J.cols), c = (int)(k % J.cols);
                J.wihT[(int64_t)c * J.rows3 + r] = J.wih[k];
                continue;
            }
            k -= nt;
        }
        if (k < nm) { J.mix_on[k] = pack_mixer_elem(J.mp, J.mo, J.mix_src_on, k, J.S, J.E, J.HE); continue; }
        k -= nm;
        if (k < nm) { J.mix_tg[k] = pack_mixer_elem(J.mp, J.mo, J.mix_src_tg, k, J.S, J.E, J.HE); continue; }
        k -= nm;
        if (k < J.n_d2) { J.d2[k] = 0.f; continue; }
        k -= J.n_d2;
        if (k < J.n_dq) { J.dq[k] = 0.f; continue; }
        k -= J.n_dq;
        // four parameters per item. Bits, not values: a NaN equals only its own copy, and -0 differs from 0
        bool ne = false;
        if (J.cmp_vec && 4 * k + 3 < J.n_cmp) {
            const uint4 a = *reinterpret_cast<const uint4*>(J.cmp_on + 4 * k);
            const uint4 b = *reinterpret_cast<const uint4*>(J.cmp_tg + 4 * k);
            ne = a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w;
        } else {
            for (int64_t e = 4 * k; e < min(4 * k + 4, J.n_cmp); ++e)
                ne = ne || __float_as_uint(J.cmp_on[e]) != __float_as_uint(J.cmp_tg[e]);
        }
        if (ne) *J.flag = 1u;
    }
}


#ifdef MLG_STAMPS
// Diagnostic build only (-DMLG_STAMPS): per-wave cycle counts of the recurrences' step phases, written to
// g_mlg_lstamps[kernel][block][wave][8] (slots 0..5 phases, 6 = steps, 7 = whole kernel).
__device__ unsigned long long* g_mlg_lstamps = nullptr;
struct LStamps {
    unsigned long long acc[6], last, begin, steps;
    __device__ void init() {
        for (int k = 0; k < 6; ++k) acc[k] = 0;
        steps = 0;
        last = begin = __builtin_amdgcn_s_memtime();
    }
    __device__ void mark(int k) {
        __builtin_amdgcn_sched_barrier(0);
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        acc[k] += now - last;
        last = now;
        __builtin_amdgcn_sched_barrier(0);
    }
    __device__ void flush(int kid) {
        if ((threadIdx.x & 63) || !g_mlg_lstamps) return;
        unsigned long long* o = g_mlg_lstamps + (((int64_t)kid * 1024 + blockIdx.x) * 8 + (threadIdx.x >> 6)) * 8;
        for (int k = 0; k < 6; ++k) o[k] = acc[k];
        o[6] = steps;
        o[7] = __builtin_amdgcn_s_memtime() - begin;
    }
};
#else
struct LStamps {
    unsigned long long steps;
    __device__ void init() {}
    __device__ void mark(int) {}
    __device__ void flush(int) {}
};
#endif

// ================================================================================================
// 16-row x 16-feature tile product with the activation operand in LDS, row-major [16][lda]:
// acc += W[m0 + col][kc*16 .. ] . act[row][kc*16 ..] over kchunks chunks.
__device__ __forceinline__ floatx4 tile_mm_lds(const float* __restrict__ W, int64_t ldw, int m0, const float* act, int lda,
                                               int kchunks, floatx4 acc, int lane) {
    const int col = lane & 15, g = lane >> 4;
    const float* wrow = W + (int64_t)(m0 + col) * ldw + 4 * g;
    const float* arow = act + col * lda + 4 * g;
    for (int kc = 0; kc < kchunks; ++kc) acc = mfma_chunk(ld4(wrow + kc * 16), ld4(arow + kc * 16), acc);
    return acc;
}


// ================================================================================================
// forward, split into the parallel (non-recurrent) and the recurrent part:
//   agent_in_kernel  (t, tile, net): dense input row (online), x = relu(fc1(inputs)), and
//                    GI = [b_ir + b_hr + W_ir x | b_iz + b_hz + W_iz x | b_in + W_in x]  for every timestep
//   agent_rec4_kernel (tile4, net):  h_t = GRU(GI_t, h_{t-1}) with W_hh in VGPRs, GI prefetched ahead
//   agent_q_kernel   (t, tile, net): q = fc2(h_t)
// The accumulation order per output is the one of the fused unroll (bias, W_ih x chunks, W_hh h chunks).
// grid (ntiles, T, 2), HC waves: wave w computes x chunk w, then GI chunks w, w + HC, w + 2 HC.
// DX (distinct networks): grid (ntiles, T, 2 N), z = 2 ag + net; instance ag's rows r = b are agent slot ag's.
template <int H, bool DX = false>
__global__ void __launch_bounds__(512) agent_in_kernel(LCfg c, MlgBatch bt, AgentLayout L, const float* __restrict__ Pon,
                                                       const float* __restrict__ Ptg, float* __restrict__ ws_in,
                                                       float* __restrict__ ws_x, float* __restrict__ gi_on,
                                                       float* __restrict__ gi_tg, Skip sk) {
    constexpr int HC = H / 16;
    constexpr int LDA = H + 4;
    __shared__ __attribute__((aligned(16))) float xs[16 * LDA];
    const int tile = blockIdx.x, t = blockIdx.y;
    if (t >= tile_steps(sk, tile)) return;
    const bool online = DX ? (blockIdx.z & 1) == 0 : blockIdx.z == 0;
    if (!online && !target_runs(c, sk)) return;
    const int ag = DX ? (int)(blockIdx.z >> 1) : 0;
    if constexpr (DX) {
        const DxView v = dx_view(c, L, ag);
        Pon += v.p, Ptg += v.p, ws_in += v.in, ws_x += v.h, gi_on += v.g3, gi_tg += v.g3;
    }
    const float* P = online ? Pon : Ptg;
    float* gi = online ? gi_on : gi_tg;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int N = c.N, A = c.A, R = DX ? c.B : c.R;
    const int r = tile * 16 + col;
    const bool valid = r < R;
    const int b = valid ? (DX ? r : r / N) : 0, n = DX ? ag : (valid ? r % N : 0);
    const int64_t boff = (bslot(bt, b) * bt.T1 + t) * N + n;
    {
        floatx4 acc = ld4(P + L.b1 + w * 16 + 4 * g);
        if (valid) {
            if (L.last_action && t > 0) {
                // the one-hot row's only possible nonzero is at the recorded action (actions_onehot = OneHot(actions),
                // zero rows past an episode's end): one load of that element instead of a scan of the A columns
                const int a = (int)bt.actions[boff - N];
                const float v = (a >= 0 && a < A) ? bt.actions_onehot[(boff - N) * A + a] : 0.f;
                if (v != 0.f) acc += v * ld4(P + L.w1a + (int64_t)a * H + w * 16 + 4 * g);
            }
            if (L.agent_id) acc += ld4(P + L.w1n + (int64_t)n * H + w * 16 + 4 * g);
        }
        const float* orow = valid ? bt.obs + boff * c.d_obs : nullptr;
        const float* wrow = P + L.w1o + (int64_t)(w * 16 + col) * L.Dob + 4 * g;
        for (int kc = 0; kc < L.Dob / 16; ++kc)
            acc = mfma_chunk(ld4(wrow + kc * 16), load_chunk(orow, kc * 16 + 4 * g, c.d_obs), acc);
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = fmaxf(acc[q], 0.f);
        *reinterpret_cast<floatx4*>(xs + col * LDA + w * 16 + 4 * g) = acc;
        if (online && valid) *reinterpret_cast<floatx4*>(ws_x + ((int64_t)t * R + r) * H + w * 16 + 4 * g) = acc;
    }
    if (online) {  // dense input row for dW1 (basic_controller.py:80-92 layout): 16 threads per row, one division per row
        const int l = tid & 15, oa = c.d_obs + (L.last_action ? A : 0);
        for (int i = tid >> 4; i < 16; i += blockDim.x >> 4) {
            const int rr = tile * 16 + i;
            if (rr >= R) break;
            const int bb = DX ? rr : rr / N, nn = DX ? ag : rr - bb * N;
            const int64_t bo = (bslot(bt, bb) * bt.T1 + t) * N + nn;
            float* dst = ws_in + ((int64_t)t * R + rr) * c.d_in;
            const float* src = bt.obs + bo * c.d_obs;
            for (int k = l; k < c.d_obs; k += 16) dst[k] = src[k];
            if (L.last_action)
                for (int k = l; k < A; k += 16) dst[c.d_obs + k] = t > 0 ? bt.actions_onehot[(bo - N) * A + k] : 0.f;
            for (int k = l; k < c.d_in - oa; k += 16) dst[oa + k] = k == nn ? 1.f : 0.f;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 3; ++q) {  // gate q, feature chunk w
        floatx4 acc = q < 2 ? ld4(P + L.brz + q * H + w * 16 + 4 * g) : ld4(P + L.bih + 2 * H + w * 16 + 4 * g);
        acc = tile_mm_lds(P + L.wih, H, q * H + w * 16, xs, LDA, HC, acc, lane);
        if (valid) *reinterpret_cast<floatx4*>(gi + ((int64_t)t * R + r) * 3 * H + q * H + w * 16 + 4 * g) = acc;
    }
}

// The recurrence on 4-row tiles with v_mfma_f32_4x4x1_16b_f32 (16 blocks of D[4x4] += A[4x1] B[1x4]; lane
// 4b + i supplies A_b[i], lane 4b + j supplies B_b[j], D_b[i][j] is register i of lane 4b + j). A 16-row tile
// per CU is MFMA-bound at 48 16x16x4 MFMAs per SIMD per step; 4-row tiles put 4x as many CUs on the
// sequential T loop. Wave w owns hidden features 16w..16w+15: block b = 4g + fg computes gate g (r, z, W_hn h;
// g = 3 idle) of features 16w + 4fg + i for the tile's 4 rows, W_hh rows of the block in VGPRs (H per lane).
// A row / register transpose across the wave's four 16-lane rows (rows_transpose4, four VALU lane swaps) then
// gives every lane the three gates of one (feature 16w + 4fg + g, row): all 64 lanes finish one GRU cell each.
// grid (2 * ntiles4): blockIdx < ntiles4 online (saves gates), else target. H/16 waves.
template <int H>
__device__ __forceinline__ void agent_rec4_body(const LCfg& c, const AgentLayout& L, const float* __restrict__ Pon,
                                                const float* __restrict__ Ptg, const float* __restrict__ gi_on,
                                                const float* __restrict__ gi_tg, float* __restrict__ hs_on,
                                                float* __restrict__ hs_tg, float* __restrict__ ws_gr,
                                                float* __restrict__ ws_gz, float* __restrict__ ws_gn,
                                                float* __restrict__ ws_ghn, const Skip& sk, int bid, int R) {
    const int nt4 = (R + 3) / 4;
    const bool online = bid < nt4;
    if (!online && !target_runs(c, sk)) return;
    LStamps lst;
    lst.init();
    const float* P = online ? Pon : Ptg;
    const mlg::Gru4Fwd a{R, P + L.whh, P + L.bhh, online ? gi_on : gi_tg, online ? hs_on : hs_tg,
                         ws_gr, ws_gz, ws_gn, ws_ghn, online};
    const int tile4 = online ? bid : bid - nt4;
    mlg::gru4_fwd<H>(a, tile4, tile_steps(sk, tile4 >> 2), lst);
    lst.flush(0);
}

// DX (distinct networks): grid (2 * ntiles4 of one instance, N), y = ag.
template <int H, bool DX = false>
__global__ void __launch_bounds__(512) agent_rec4_kernel(LCfg c, AgentLayout L, const float* __restrict__ Pon,
                                                         const float* __restrict__ Ptg, const float* __restrict__ gi_on,
                                                         const float* __restrict__ gi_tg, float* __restrict__ hs_on,
                                                         float* __restrict__ hs_tg, float* __restrict__ ws_gr,
                                                         float* __restrict__ ws_gz, float* __restrict__ ws_gn,
                                                         float* __restrict__ ws_ghn, Skip sk) {
    if constexpr (DX) {
        const DxView v = dx_view(c, L, blockIdx.y);
        agent_rec4_body<H>(c, L, Pon + v.p, Ptg + v.p, gi_on + v.g3, gi_tg + v.g3, hs_on + v.hs, hs_tg + v.hs,
                           ws_gr + v.h, ws_gz + v.h, ws_gn + v.h, ws_ghn + v.h, sk, blockIdx.x, c.B);
    } else {
        agent_rec4_body<H>(c, L, Pon, Ptg, gi_on, gi_tg, hs_on, hs_tg, ws_gr, ws_gz, ws_gn, ws_ghn, sk, blockIdx.x, c.R);
    }
}

// grid (ntiles, T, 2), Ap/16 waves: wave = action tile. q = b2 + W2 . h_t (h_t = HS[t + 1]).
// DX (distinct networks): grid (ntiles, T, 2 N), z = 2 ag + net; instance row r = b stores to the mixer's row b N + ag.
template <int H, bool DX = false>
__global__ void __launch_bounds__(512) agent_q_kernel(LCfg c, AgentLayout L, const float* __restrict__ Pon,
                                                      const float* __restrict__ Ptg, const float* __restrict__ hs_on,
                                                      const float* __restrict__ hs_tg, float* __restrict__ mac,
                                                      float* __restrict__ tmac, Skip sk) {
    constexpr int HC = H / 16;
    const int tile = blockIdx.x, t = blockIdx.y;
    if (t >= tile_steps(sk, tile)) return;
    const bool online = DX ? (blockIdx.z & 1) == 0 : blockIdx.z == 0;
    if (!online && !target_runs(c, sk)) return;
    const int ag = DX ? (int)(blockIdx.z >> 1) : 0;
    if constexpr (DX) {
        const DxView v = dx_view(c, L, ag);
        Pon += v.p, Ptg += v.p, hs_on += v.hs, hs_tg += v.hs;
    }
    const int R = DX ? c.B : c.R;
    const float* P = online ? Pon : Ptg;
    const float* hsg = (online ? hs_on : hs_tg) + (int64_t)(t + 1) * R * H;
    float* qout = online ? mac : tmac;
    const int lane = threadIdx.x & 63, at = threadIdx.x >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int r = tile * 16 + col;
    const bool valid = r < R;
    const float* hrow = hsg + (int64_t)(valid ? r : 0) * H + 4 * g;
    const float* wrow = P + L.w2 + (int64_t)(at * 16 + col) * H + 4 * g;
    floatx4 q = ld4(P + L.b2 + at * 16 + 4 * g);
#pragma unroll
    for (int kc = 0; kc < HC; ++kc) q = mfma_chunk(ld4(wrow + kc * 16), ld4(hrow + kc * 16), q);
    if (valid) {
        const int64_t qrow = DX ? (int64_t)t * c.R + r * c.N + ag : (int64_t)t * c.R + r;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int a = at * 16 + 4 * g + k;
            if (a < c.A) qout[qrow * c.A + a] = q[k];
        }
    }
}

// ================================================================================================
// Feed-forward agent (cfg.agent = 1): no recurrence, so the hidden rows of every (tile, t) block are independent.
//   ff_hidden_kernel (t, tile, net): x = relu(fc1(inputs)) into the hidden rows agent_q_kernel reads (row block t + 1
//                    of hs / hs_tg), and for the online net the dense input row the fc1 weight-gradient job reads.
//                    agent_in_kernel's fc1 part, line for line: the same sums in the same order.
//   ff_bwd_kernel    (t, tile): dh = W2^T d2 (d2 [T][R][A], the mixer's deltas), masked by the ReLU -> the fc1 delta rows.
// grid (ntiles, T, 2) / (ntiles, T), HC waves: wave w computes feature chunk w.
template <int H>
__global__ void __launch_bounds__(512) ff_hidden_kernel(LCfg c, MlgBatch bt, AgentLayout L, const float* __restrict__ Pon,
                                                        const float* __restrict__ Ptg, float* __restrict__ ws_in,
                                                        float* __restrict__ hs_on, float* __restrict__ hs_tg, Skip sk) {
    const int tile = blockIdx.x, t = blockIdx.y;
    if (t >= tile_steps(sk, tile)) return;
    const bool online = blockIdx.z == 0;
    if (!online && !target_runs(c, sk)) return;
    const float* P = online ? Pon : Ptg;
    float* hs = (online ? hs_on : hs_tg) + (int64_t)(t + 1) * c.R * H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int N = c.N, A = c.A, R = c.R;
    const int r = tile * 16 + col;
    const bool valid = r < R;
    const int b = valid ? r / N : 0, n = valid ? r % N : 0;
    const int64_t boff = (bslot(bt, b) * bt.T1 + t) * N + n;
    floatx4 acc = ld4(P + L.b1 + w * 16 + 4 * g);
    if (valid) {
        if (L.last_action && t > 0) {
            const int a = (int)bt.actions[boff - N];
            const float v = (a >= 0 && a < A) ? bt.actions_onehot[(boff - N) * A + a] : 0.f;
            if (v != 0.f) acc += v * ld4(P + L.w1a + (int64_t)a * H + w * 16 + 4 * g);
        }
        if (L.agent_id) acc += ld4(P + L.w1n + (int64_t)n * H + w * 16 + 4 * g);
    }
    const float* orow = valid ? bt.obs + boff * c.d_obs : nullptr;
    const float* wrow = P + L.w1o + (int64_t)(w * 16 + col) * L.Dob + 4 * g;
    for (int kc = 0; kc < L.Dob / 16; ++kc)
        acc = mfma_chunk(ld4(wrow + kc * 16), load_chunk(orow, kc * 16 + 4 * g, c.d_obs), acc);
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = fmaxf(acc[q], 0.f);
    if (valid) *reinterpret_cast<floatx4*>(hs + (int64_t)r * H + w * 16 + 4 * g) = acc;
    if (!online) return;
    // dense input row for dW1 (basic_controller.py:80-92 layout): 16 threads per row
    const int l = tid & 15, oa = c.d_obs + (L.last_action ? A : 0);
    for (int i = tid >> 4; i < 16; i += blockDim.x >> 4) {
        const int rr = tile * 16 + i;
        if (rr >= R) break;
        const int bb = rr / N, nn = rr - bb * N;
        const int64_t bo = (bslot(bt, bb) * bt.T1 + t) * N + nn;
        float* dst = ws_in + ((int64_t)t * R + rr) * c.d_in;
        const float* src = bt.obs + bo * c.d_obs;
        for (int k = l; k < c.d_obs; k += 16) dst[k] = src[k];
        if (L.last_action)
            for (int k = l; k < A; k += 16) dst[c.d_obs + k] = t > 0 ? bt.actions_onehot[(bo - N) * A + k] : 0.f;
        for (int k = l; k < c.d_in - oa; k += 16) dst[oa + k] = k == nn ? 1.f : 0.f;
    }
}

template <int H>
__global__ void __launch_bounds__(512) ff_bwd_kernel(LCfg c, AgentLayout L, const float* __restrict__ P,
                                                     const float* __restrict__ hs_on, const float* __restrict__ d2,
                                                     float* __restrict__ da, Skip sk) {
    const int tile = blockIdx.x, t = blockIdx.y;
    if (t >= tile_steps(sk, tile)) return;  // the fc1 weight gradient skips the block's rows
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int r = tile * 16 + col;
    const bool valid = r < c.R;
    const int64_t row = (int64_t)t * c.R + (valid ? r : 0);
    const float* drow = valid ? d2 + row * c.A : nullptr;
    const floatx4 xv = ld4(hs_on + (int64_t)(t + 1) * c.R * H + (int64_t)(valid ? r : 0) * H + w * 16 + 4 * g);
    floatx4 dh = {0.f, 0.f, 0.f, 0.f};
    for (int at = 0; at < L.Ap / 16; ++at)  // fc2 rows past A are zero in the packed block
        dh = mfma_chunk(ld_col4(P + L.w2, at * 16 + 4 * g, H, w * 16 + col), load_chunk(drow, at * 16 + 4 * g, c.A), dh);
    if (valid) {
#pragma unroll
        for (int q = 0; q < 4; ++q) dh[q] = xv[q] > 0.f ? dh[q] : 0.f;
        *reinterpret_cast<floatx4*>(da + row * H + w * 16 + 4 * g) = dh;
    }
}

// ================================================================================================
// QMixer on one 16-row tile (rows on lanes).  l1 = [w1h | wfh | b1 | vh] (post ReLU except b1).
template <int HE, int E>
struct Mixer {
    static constexpr int T1H = HE / 16, TE = E / 16, L1T = (2 * HE + 2 * E) / 16;
    static constexpr int OW1 = 0, OWF = T1H, OB1 = 2 * T1H, OVH = 2 * T1H + TE;

    // first layer + ReLUs; s = this lane's state row (nullptr -> zeros)
    __device__ static void layer1(const MixPtrs& M, const MixPack& mp, int S, const float* s, floatx4 (&l1)[L1T], int lane) {
        const int col = lane & 15, g = lane >> 4;
#pragma unroll
        for (int mt = 0; mt < L1T; ++mt) l1[mt] = ld4(M.mb1 + mt * 16 + 4 * g);
        for (int kc = 0; kc < mp.Sp / 16; ++kc) {
            const floatx4 sv = load_chunk(s, kc * 16 + 4 * g, S);
#pragma unroll
            for (int mt = 0; mt < L1T; ++mt)
                l1[mt] = mfma_chunk(ld4(M.m1 + (int64_t)(mt * 16 + col) * mp.Sp + kc * 16 + 4 * g), sv, l1[mt]);
        }
#pragma unroll
        for (int mt = 0; mt < L1T; ++mt) {
            if (mt >= OB1 && mt < OVH) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) l1[mt][q] = fmaxf(l1[mt][q], 0.f);
        }
    }

    // pre-abs hyper_w_1 output for agent n, chunk cc (features n*E + cc*16 ..)
    __device__ static floatx4 w1pre(const MixPtrs& M, int n, int cc, const floatx4 (&l1)[L1T], int lane) {
        const int col = lane & 15, g = lane >> 4;
        floatx4 acc = ld4(M.ba2 + n * E + cc * 16 + 4 * g);
        const float* wrow = M.a2 + (int64_t)(n * E + cc * 16 + col) * HE + 4 * g;
#pragma unroll
        for (int kc = 0; kc < T1H; ++kc) acc = mfma_chunk(ld4(wrow + kc * 16), l1[OW1 + kc], acc);
        return acc;
    }

    __device__ static floatx4 wfpre(const MixPtrs& M, int cc, const floatx4 (&l1)[L1T], int lane) {
        const int col = lane & 15, g = lane >> 4;
        floatx4 acc = ld4(M.bf2 + cc * 16 + 4 * g);
        const float* wrow = M.f2 + (int64_t)(cc * 16 + col) * HE + 4 * g;
#pragma unroll
        for (int kc = 0; kc < T1H; ++kc) acc = mfma_chunk(ld4(wrow + kc * 16), l1[OWF + kc], acc);
        return acc;
    }

    __device__ static float vval(const MixPtrs& M, const floatx4 (&l1)[L1T], int lane) {
        const int col = lane & 15, g = lane >> 4;
        floatx4 acc = ld4(M.bv2p + 4 * g);
        const float* wrow = M.v2p + (int64_t)col * E + 4 * g;
#pragma unroll
        for (int kc = 0; kc < TE; ++kc) acc = mfma_chunk(ld4(wrow + kc * 16), l1[OVH + kc], acc);
        return __shfl(acc[0], col);  // feature 0 lives in lane group 0, reg 0
    }

    // forward: y per row (identical in the 4 lanes of a row). q(n) = this row's agent-n value.
    __device__ static float forward(const MixPtrs& M, const MixPack& mp, int S, int N, const float* s, const float* qrow,
                                    floatx4 (&l1)[L1T], floatx4 (&pre)[TE], floatx4 (&hid)[TE], floatx4 (&wfp)[TE], int lane) {
        layer1(M, mp, S, s, l1, lane);
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) pre[cc] = l1[OB1 + cc];
        for (int n = 0; n < N; ++n) {
            const float qn = qrow[n];
#pragma unroll
            for (int cc = 0; cc < TE; ++cc) {
                const floatx4 wp = w1pre(M, n, cc, l1, lane);
#pragma unroll
                for (int q = 0; q < 4; ++q) pre[cc][q] += qn * fabsf(wp[q]);
            }
        }
        float part = 0.f;
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) {
            wfp[cc] = wfpre(M, cc, l1, lane);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                hid[cc][q] = pre[cc][q] > 0.f ? pre[cc][q] : expm1f(pre[cc][q]);
                part += hid[cc][q] * fabsf(wfp[cc][q]);
            }
        }
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        return part + vval(M, l1, lane);
    }
};

// The same QMixer forward with every weight operand of a stage loaded up front (one L2 round trip per stage
// instead of one per 16-wide K chunk: the mix_td waves are L2-latency-bound, one wave per SIMD, so registers are
// plentiful). State rows of at most SPC * 16 features, at most NMAX agents; identical arithmetic to Mixer. w1p
// keeps the pre-abs hyper_w_1 outputs for the backward.
template <int HE, int E, int SPC, int NMAX>
struct MixerPF {
    using Mx = Mixer<HE, E>;
    static constexpr int T1H = Mx::T1H, TE = Mx::TE, L1T = Mx::L1T;
    static constexpr int OW1 = Mx::OW1, OWF = Mx::OWF, OB1 = Mx::OB1, OVH = Mx::OVH;

    // The state-only half of forward(): layer 1, hyper_w_1's second layer for every agent (pre-abs), hyper_w_final's
    // second layer (pre-abs) and V(s) (identical in the 4 lanes of a row). Same operations as forward().
    __device__ static void hyper(const MixPtrs& M, const MixPack& mp, int S, int N, const float* s, floatx4 (&l1)[L1T],
                                 floatx4 (&w1p)[NMAX][TE], floatx4 (&wfp)[TE], float& v, int lane) {
        const int col = lane & 15, g = lane >> 4;
        {  // layer 1
            floatx4 sv[SPC], wl[L1T][SPC];
#pragma unroll
            for (int kc = 0; kc < SPC; ++kc) sv[kc] = load_chunk(s, kc * 16 + 4 * g, S);
#pragma unroll
            for (int mt = 0; mt < L1T; ++mt) {
                l1[mt] = ld4(M.mb1 + mt * 16 + 4 * g);
#pragma unroll
                for (int kc = 0; kc < SPC; ++kc) wl[mt][kc] = ld4(M.m1 + (int64_t)(mt * 16 + col) * mp.Sp + kc * 16 + 4 * g);
            }
#pragma unroll
            for (int kc = 0; kc < SPC; ++kc)
#pragma unroll
                for (int mt = 0; mt < L1T; ++mt) l1[mt] = mfma_chunk(wl[mt][kc], sv[kc], l1[mt]);
#pragma unroll
            for (int mt = 0; mt < L1T; ++mt) {
                if (mt >= OB1 && mt < OVH) continue;
#pragma unroll
                for (int q = 0; q < 4; ++q) l1[mt][q] = fmaxf(l1[mt][q], 0.f);
            }
        }
#pragma unroll
        for (int n = 0; n < NMAX; ++n) {
            if (n >= N) break;
            floatx4 wa[TE][T1H];
#pragma unroll
            for (int cc = 0; cc < TE; ++cc) {
                w1p[n][cc] = ld4(M.ba2 + n * E + cc * 16 + 4 * g);
#pragma unroll
                for (int kc = 0; kc < T1H; ++kc)
                    wa[cc][kc] = ld4(M.a2 + (int64_t)(n * E + cc * 16 + col) * HE + kc * 16 + 4 * g);
            }
#pragma unroll
            for (int cc = 0; cc < TE; ++cc)
#pragma unroll
                for (int kc = 0; kc < T1H; ++kc) w1p[n][cc] = mfma_chunk(wa[cc][kc], l1[OW1 + kc], w1p[n][cc]);
        }
        floatx4 wf[TE][T1H], wv[TE];
        floatx4 bv = ld4(M.bv2p + 4 * g);
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) {
            wfp[cc] = ld4(M.bf2 + cc * 16 + 4 * g);
            wv[cc] = ld4(M.v2p + (int64_t)col * E + cc * 16 + 4 * g);
#pragma unroll
            for (int kc = 0; kc < T1H; ++kc) wf[cc][kc] = ld4(M.f2 + (int64_t)(cc * 16 + col) * HE + kc * 16 + 4 * g);
        }
#pragma unroll
        for (int cc = 0; cc < TE; ++cc)
#pragma unroll
            for (int kc = 0; kc < T1H; ++kc) wfp[cc] = mfma_chunk(wf[cc][kc], l1[OWF + kc], wfp[cc]);
#pragma unroll
        for (int kc = 0; kc < TE; ++kc) bv = mfma_chunk(wv[kc], l1[OVH + kc], bv);
        v = __shfl(bv[0], col);
    }

    // The Q-dependent half: the mixing with hyper()'s outputs (b1 = layer-1 tiles OB1..), forward()'s order.
    __device__ static float mix(int N, const float* qrow, const floatx4 (&b1)[TE], const floatx4 (&w1p)[NMAX][TE],
                                const floatx4 (&wfp)[TE], float v, floatx4 (&pre)[TE], floatx4 (&hid)[TE]) {
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) pre[cc] = b1[cc];
#pragma unroll
        for (int n = 0; n < NMAX; ++n) {
            if (n >= N) break;
            const float qn = qrow[n];
#pragma unroll
            for (int cc = 0; cc < TE; ++cc)
#pragma unroll
                for (int q = 0; q < 4; ++q) pre[cc][q] += qn * fabsf(w1p[n][cc][q]);
        }
        float part = 0.f;
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                hid[cc][q] = pre[cc][q] > 0.f ? pre[cc][q] : expm1f(pre[cc][q]);
                part += hid[cc][q] * fabsf(wfp[cc][q]);
            }
        }
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        return part + v;
    }

    __device__ static float forward(const MixPtrs& M, const MixPack& mp, int S, int N, const float* s, const float* qrow,
                                    floatx4 (&l1)[L1T], floatx4 (&pre)[TE], floatx4 (&hid)[TE], floatx4 (&wfp)[TE],
                                    floatx4 (&w1p)[NMAX][TE], int lane) {
        const int col = lane & 15, g = lane >> 4;
        {  // layer 1
            floatx4 sv[SPC], wl[L1T][SPC];
#pragma unroll
            for (int kc = 0; kc < SPC; ++kc) sv[kc] = load_chunk(s, kc * 16 + 4 * g, S);
#pragma unroll
            for (int mt = 0; mt < L1T; ++mt) {
                l1[mt] = ld4(M.mb1 + mt * 16 + 4 * g);
#pragma unroll
                for (int kc = 0; kc < SPC; ++kc) wl[mt][kc] = ld4(M.m1 + (int64_t)(mt * 16 + col) * mp.Sp + kc * 16 + 4 * g);
            }
#pragma unroll
            for (int kc = 0; kc < SPC; ++kc)
#pragma unroll
                for (int mt = 0; mt < L1T; ++mt) l1[mt] = mfma_chunk(wl[mt][kc], sv[kc], l1[mt]);
#pragma unroll
            for (int mt = 0; mt < L1T; ++mt) {
                if (mt >= OB1 && mt < OVH) continue;
#pragma unroll
                for (int q = 0; q < 4; ++q) l1[mt][q] = fmaxf(l1[mt][q], 0.f);
            }
        }
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) pre[cc] = l1[OB1 + cc];
#pragma unroll
        for (int n = 0; n < NMAX; ++n) {  // hyper_w_1 second layer for every agent: weights of all agents first
            if (n >= N) break;
            floatx4 wa[TE][T1H];
#pragma unroll
            for (int cc = 0; cc < TE; ++cc) {
                w1p[n][cc] = ld4(M.ba2 + n * E + cc * 16 + 4 * g);
#pragma unroll
                for (int kc = 0; kc < T1H; ++kc)
                    wa[cc][kc] = ld4(M.a2 + (int64_t)(n * E + cc * 16 + col) * HE + kc * 16 + 4 * g);
            }
#pragma unroll
            for (int cc = 0; cc < TE; ++cc)
#pragma unroll
                for (int kc = 0; kc < T1H; ++kc) w1p[n][cc] = mfma_chunk(wa[cc][kc], l1[OW1 + kc], w1p[n][cc]);
        }
#pragma unroll
        for (int n = 0; n < NMAX; ++n) {
            if (n >= N) break;
            const float qn = qrow[n];
#pragma unroll
            for (int cc = 0; cc < TE; ++cc)
#pragma unroll
                for (int q = 0; q < 4; ++q) pre[cc][q] += qn * fabsf(w1p[n][cc][q]);
        }
        floatx4 wf[TE][T1H], wv[TE];
        floatx4 bv = ld4(M.bv2p + 4 * g);
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) {
            wfp[cc] = ld4(M.bf2 + cc * 16 + 4 * g);
            wv[cc] = ld4(M.v2p + (int64_t)col * E + cc * 16 + 4 * g);
#pragma unroll
            for (int kc = 0; kc < T1H; ++kc) wf[cc][kc] = ld4(M.f2 + (int64_t)(cc * 16 + col) * HE + kc * 16 + 4 * g);
        }
        float part = 0.f;
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) {
#pragma unroll
            for (int kc = 0; kc < T1H; ++kc) wfp[cc] = mfma_chunk(wf[cc][kc], l1[OWF + kc], wfp[cc]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                hid[cc][q] = pre[cc][q] > 0.f ? pre[cc][q] : expm1f(pre[cc][q]);
                part += hid[cc][q] * fabsf(wfp[cc][q]);
            }
        }
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
#pragma unroll
        for (int kc = 0; kc < TE; ++kc) bv = mfma_chunk(wv[kc], l1[OVH + kc], bv);
        return part + __shfl(bv[0], col);
    }
};

__device__ __forceinline__ float row_sum16(float v) {  // sum over the 16 lanes of lane group 0
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    return v;
}

// chosen / target per-agent values of row (b, t) (q_learner.py:55, 68-75)
__device__ __forceinline__ void gather_q1(const LCfg& c, const MlgBatch& bt, const float* mac, const float* tmac, int b,
                                          int t, int n, int& act, float& cq, float& tq) {
    const int N = c.N, A = c.A, R = c.R;
    const int r = b * N + n;
    const int a = (int)bt.actions[(bslot(bt, b) * bt.T1 + t) * N + n];
    act = a;
    cq = mac[((int64_t)t * R + r) * A + a];
    const int32_t* av = bt.avail + (bslot(bt, b) * bt.T1 + t + 1) * N * A + (int64_t)n * A;
    const float* qn = mac + ((int64_t)(t + 1) * R + r) * A;
    const float* tn = tmac + ((int64_t)(t + 1) * R + r) * A;
    if (c.double_q) {
        float bv = 0.f;
        int bi = 0;
        for (int k = 0; k < A; ++k) {
            const float v = av[k] ? qn[k] : -9999999.f;
            if (k == 0 || v > bv) { bv = v; bi = k; }
        }
        tq = av[bi] ? tn[bi] : -9999999.f;
    } else {
        float bv = 0.f;
        for (int k = 0; k < A; ++k) {
            const float v = av[k] ? tn[k] : -9999999.f;
            if (k == 0 || v > bv) bv = v;
        }
        tq = bv;
    }
}

__device__ __forceinline__ void gather_q(const LCfg& c, const MlgBatch& bt, const float* mac, const float* tmac, int b, int t,
                                         float* cq, float* tq) {
    for (int n = 0; n < c.N; ++n) {
        int a;
        gather_q1(c, bt, mac, tmac, b, t, n, a, cq[n], tq[n]);
    }
}

constexpr int MIXPF_N = 8, MIXPF_A = 16;  // mix_td FAST path bounds (agents, actions)

// gather_q with every load of an agent issued together (A <= AMAX): avail row, online next-step Q, target
// next-step Q; same selection rule and order as gather_q.
template <int AMAX>
__device__ __forceinline__ void gather_q_pf(const LCfg& c, const MlgBatch& bt, const float* mac, const float* tmac, int b,
                                            int t, float* cq, float* tq) {
    const int N = c.N, A = c.A, R = c.R;
    const int64_t row0 = (bslot(bt, b) * bt.T1 + t) * N;
#pragma unroll
    for (int n = 0; n < MIXPF_N; ++n) {  // unrolled: cq / tq stay in registers
        if (n >= N) break;
        const int r = b * N + n;
        const int a = (int)bt.actions[row0 + n];
        const int32_t* av = bt.avail + (bslot(bt, b) * bt.T1 + t + 1) * N * A + (int64_t)n * A;
        const float* qn = mac + ((int64_t)(t + 1) * R + r) * A;
        const float* tn = tmac + ((int64_t)(t + 1) * R + r) * A;
        int avv[AMAX];
        float qv[AMAX], tv[AMAX];
#pragma unroll
        for (int k = 0; k < AMAX; ++k) {
            const bool in = k < A;
            avv[k] = in ? av[k] : 0;
            qv[k] = in ? qn[k] : 0.f;
            tv[k] = in ? tn[k] : 0.f;
        }
        cq[n] = mac[((int64_t)t * R + r) * A + a];
        if (c.double_q) {
            float bv = 0.f;
            int bi = 0;
#pragma unroll
            for (int k = 0; k < AMAX; ++k) {
                if (k >= A) break;
                const float v = avv[k] ? qv[k] : -9999999.f;
                const bool take = k == 0 || v > bv;
                bv = take ? v : bv;
                bi = take ? k : bi;
            }
            float tb = 0.f;
            int ab = 0;
#pragma unroll
            for (int k = 0; k < AMAX; ++k) {  // tv[bi], avv[bi] without dynamic register indexing
                tb = k == bi ? tv[k] : tb;
                ab = k == bi ? avv[k] : ab;
            }
            tq[n] = ab ? tb : -9999999.f;
        } else {
            float bv = 0.f;
#pragma unroll
            for (int k = 0; k < AMAX; ++k) {
                if (k >= A) break;
                const float v = avv[k] ? tv[k] : -9999999.f;
                bv = (k == 0 || v > bv) ? v : bv;
            }
            tq[n] = bv;
        }
    }
}

constexpr int MAXN = 32;

// gather_q_pf with the agents spread over the four 16-lane rows (row g takes agents g, g + 4, ...: the rows of a D
// layout hold the same (b, t) row, so gather_q_pf loaded everything four times) and the values all-gathered back by
// rows_transpose4 (VALU lane swaps). Same selection rule per agent; N <= 8.
template <int AMAX>
__device__ __forceinline__ void gather_q_rows(const LCfg& c, const MlgBatch& bt, const float* mac, const float* tmac, int b,
                                              int t, bool valid, int g, float* cq, float* tq) {
    const int N = c.N, A = c.A, R = c.R;
    const int64_t row0 = (bslot(bt, b) * bt.T1 + t) * N;
    float cv[2], tv[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = g + 4 * i;
        cv[i] = tv[i] = 0.f;
        if (!valid || n >= N) continue;
        const int r = b * N + n;
        const int a = (int)bt.actions[row0 + n];
        const int32_t* av = bt.avail + (bslot(bt, b) * bt.T1 + t + 1) * N * A + (int64_t)n * A;
        const float* qn = mac + ((int64_t)(t + 1) * R + r) * A;
        const float* tn = tmac + ((int64_t)(t + 1) * R + r) * A;
        int avv[AMAX];
        float qv[AMAX], tvv[AMAX];
#pragma unroll
        for (int k = 0; k < AMAX; ++k) {
            const bool in = k < A;
            avv[k] = in ? av[k] : 0;
            qv[k] = in ? qn[k] : 0.f;
            tvv[k] = in ? tn[k] : 0.f;
        }
        cv[i] = mac[((int64_t)t * R + r) * A + a];
        if (c.double_q) {
            float bv = 0.f;
            int bi = 0;
#pragma unroll
            for (int k = 0; k < AMAX; ++k) {
                if (k >= A) break;
                const float v = avv[k] ? qv[k] : -9999999.f;
                const bool take = k == 0 || v > bv;
                bv = take ? v : bv;
                bi = take ? k : bi;
            }
            float tb = 0.f;
            int ab = 0;
#pragma unroll
            for (int k = 0; k < AMAX; ++k) {
                tb = k == bi ? tvv[k] : tb;
                ab = k == bi ? avv[k] : ab;
            }
            tv[i] = ab ? tb : -9999999.f;
        } else {
            float bv = 0.f;
#pragma unroll
            for (int k = 0; k < AMAX; ++k) {
                if (k >= A) break;
                const float v = avv[k] ? tvv[k] : -9999999.f;
                bv = (k == 0 || v > bv) ? v : bv;
            }
            tv[i] = bv;
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {  // row p's value of agent p + 4 i to every row
        float c0 = cv[i], c1 = cv[i], c2 = cv[i], c3 = cv[i];
        float t0 = tv[i], t1 = tv[i], t2 = tv[i], t3 = tv[i];
        rows_transpose4(c0, c1, c2, c3);
        rows_transpose4(t0, t1, t2, t3);
        const float cs[4] = {c0, c1, c2, c3}, ts[4] = {t0, t1, t2, t3};
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (4 * i + p >= MIXPF_N) break;
            cq[4 * i + p] = cs[p];
            tq[4 * i + p] = ts[p];
        }
    }
}

struct MixOut {
    float *srow, *l1act, *d1, *da2, *df2, *dv2, *dq, *d2, *part;
};

// Prioritized replay (MlgLearnerCfg.per = 1): the PER = true form of each TD kernel scales d loss /
// d q_tot and the loss partial of episode b by w[b] and stores each live row's masked |td| (IQL: summed over the row's
// agents) to tdrow [RM]; per_reduce_kernel then adds an episode's rows. The PER = false forms read neither pointer and
// are the instantiations an unweighted call has always launched. With w = 1 the arithmetic has the same bits: 2 * 1 and
// 1 * x are exact.
struct PerIo {
    const float* w;
    float* tdrow;
};

// FAST (state rows of <= 64 features, <= 8 agents, <= 16 actions): the prefetching mixer forward (MixerPF), the
// backward reusing its hyper_w_1 outputs with the W_a2^T / W_f2^T operands loaded up front, gather_q_pf.
// Identical arithmetic either way.
template <int HE, int E, bool FAST = false, bool PER = false>
__global__ void __launch_bounds__(128) mix_td_kernel(LCfg c, MlgBatch bt, MixPtrs Mon, MixPtrs Mtg, MixPack mp,
                                                    const float* __restrict__ mac, const float* __restrict__ tmac_,
                                                    const float* __restrict__ msum_p, MixOut o, Skip sk, PerIo pw) {
    using Mx = Mixer<HE, E>;
    using MP = MixerPF<HE, E, 4, MIXPF_N>;
    floatx4 w1c[MIXPF_N][Mx::TE];  // FAST: the online forward's pre-abs hyper_w_1 outputs
    // two waves per 16-row tile: wave 0 runs the target mixer forward and hands y's target to wave 1 through LDS,
    // wave 1 runs the online forward, TD and the mixer backward (VDN: wave 1 alone)
    __shared__ float tgt_sh[16];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    if (c.mixer != 2 && wv == 0) return;
    const int rm = blockIdx.x * 16 + col;
    const int Tm = c.T - 1;
    const bool valid = rm < c.RM;
    const int b = valid ? rm / Tm : 0, t = valid ? rm % Tm : 0;
    const int N = c.N, S = c.S, L1 = 2 * HE + 2 * E, NE = N * E;
    // a dead transition (Skip::mlen) has mask 0: it takes zeros for its Qs and state, stores nothing (the weight
    // gradients skip its rows, dq / d2 keep prep_kernel's zeros) and adds exact zeros to the tile's sums
    const bool live = valid && t < (int)sk.mlen[b];
    if (!__any(live)) {  // both waves of the tile alike
        if (wv == 1 && lane < 4) o.part[(int64_t)blockIdx.x * 4 + lane] = 0.f;
        return;
    }
    const bool tr = target_runs(c, sk);  // else the online buffers hold the target's bits
    const float* tmac = tr ? tmac_ : mac;
    const MixPtrs& Mt = tr ? Mtg : Mon;
    float cq[MAXN], tq[MAXN];
    for (int n = 0; n < N; ++n) cq[n] = tq[n] = 0.f;
    if (live) {
        if constexpr (FAST)
            gather_q_pf<MIXPF_A>(c, bt, mac, tmac, b, t, cq, tq);
        else
            gather_q(c, bt, mac, tmac, b, t, cq, tq);
    }
    const float m = live ? mask_at(bt, b, t) : 0.f;  // reference truncation: mlen <= t_eff - 1
    const float rwd = valid ? bt.reward[bslot(bt, b) * bt.T1 + t] : 0.f;
    const float term = valid ? (float)bt.terminated[bslot(bt, b) * bt.T1 + t] : 0.f;
    const float msum = msum_p[0];
    const float* s0 = live ? bt.state + (bslot(bt, b) * bt.T1 + t) * S : nullptr;
    const float* s1 = live ? bt.state + (bslot(bt, b) * bt.T1 + t + 1) * S : nullptr;
    float qtot, tgt;
    floatx4 l1[Mx::L1T], pre[Mx::TE], hid[Mx::TE], wfp[Mx::TE];
    if (c.mixer == 2) {
        if (wv == 0) {
            floatx4 tl1[Mx::L1T], tpre[Mx::TE], thid[Mx::TE], twfp[Mx::TE];
            float tv;
            if constexpr (FAST) {
                floatx4 tw1c[MIXPF_N][Mx::TE];
                tv = MP::forward(Mt, mp, S, N, s1, tq, tl1, tpre, thid, twfp, tw1c, lane);
            } else {
                tv = Mx::forward(Mt, mp, S, N, s1, tq, tl1, tpre, thid, twfp, lane);
            }
            if (g == 0) tgt_sh[col] = tv;
            qtot = 0.f;
        } else {
            if constexpr (FAST)
                qtot = MP::forward(Mon, mp, S, N, s0, cq, l1, pre, hid, wfp, w1c, lane);
            else
                qtot = Mx::forward(Mon, mp, S, N, s0, cq, l1, pre, hid, wfp, lane);
        }
        __syncthreads();
        if (wv == 0) return;
        tgt = tgt_sh[col];
    } else {  // VDN (vdn.py:9)
        qtot = 0.f;
        tgt = 0.f;
        for (int n = 0; n < N; ++n) {
            qtot += cq[n];
            tgt += tq[n];
        }
    }
    const float y = rwd + c.gamma * (1.f - term) * tgt;          // q_learner.py:86
    const float mtd = (qtot - y) * m;                             // :89-95
    float dy = 2.f * mtd * m / msum;                              // d loss / d q_tot
    float wb = 1.f;
    if constexpr (PER) {  // the weighted loss; this row's share of its episode's error
        wb = pw.w[b];
        dy = 2.f * wb * mtd * m / msum;
        if (live && g == 0) pw.tdrow[rm] = fabsf(mtd);
    }
    // ---- loss / stat partials (one row per lane of group 0) ----
    {
        float p0 = g == 0 ? (PER ? wb * (mtd * mtd) : mtd * mtd) : 0.f, p1 = g == 0 ? fabsf(mtd) : 0.f;
        float p2 = g == 0 ? qtot * m : 0.f, p3 = g == 0 ? y * m : 0.f;
        p0 = row_sum16(p0);
        p1 = row_sum16(p1);
        p2 = row_sum16(p2);
        p3 = row_sum16(p3);
        if (lane == 0) {
            float* pp = o.part + (int64_t)blockIdx.x * 4;
            pp[0] = p0;
            pp[1] = p1;
            pp[2] = p2;
            pp[3] = p3;
        }
    }
    float dq[MAXN];
    if (c.mixer == 2) {
        // ---- QMixer backward (autograd of qmix.py:41-59) ----
        floatx4 dpre[Mx::TE], dwf[Mx::TE];
#pragma unroll
        for (int cc = 0; cc < Mx::TE; ++cc) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float dh = dy * fabsf(wfp[cc][q]);
                const float sg = wfp[cc][q] > 0.f ? 1.f : (wfp[cc][q] < 0.f ? -1.f : 0.f);
                dwf[cc][q] = dy * hid[cc][q] * sg;
                dpre[cc][q] = pre[cc][q] > 0.f ? dh : dh * (hid[cc][q] + 1.f);
            }
        }
        floatx4 dw1h[Mx::T1H];
#pragma unroll
        for (int mt = 0; mt < Mx::T1H; ++mt) dw1h[mt] = floatx4{0.f, 0.f, 0.f, 0.f};
        for (int n = 0; n < N; ++n) {
            float part = 0.f;
            floatx4 aT[Mx::TE][Mx::T1H];  // FAST: this agent's W_a2^T operands, loaded before its MFMAs
            if constexpr (FAST) {
#pragma unroll
                for (int cc = 0; cc < Mx::TE; ++cc)
#pragma unroll
                    for (int mt = 0; mt < Mx::T1H; ++mt)
                        aT[cc][mt] = ld4(Mon.a2T + (int64_t)(mt * 16 + col) * NE + n * E + cc * 16 + 4 * g);
            }
#pragma unroll
            for (int cc = 0; cc < Mx::TE; ++cc) {
                floatx4 wp;
                if constexpr (FAST) {
                    floatx4 wsel = w1c[0][cc];  // w1c[n][cc] without dynamic register indexing
#pragma unroll
                    for (int k = 1; k < MIXPF_N; ++k)
                        if (k == n) wsel = w1c[k][cc];
                    wp = wsel;
                } else {
                    wp = Mx::w1pre(Mon, n, cc, l1, lane);
                }
                floatx4 dlt;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    part += fabsf(wp[q]) * dpre[cc][q];
                    const float sg = wp[q] > 0.f ? 1.f : (wp[q] < 0.f ? -1.f : 0.f);
                    dlt[q] = cq[n] * dpre[cc][q] * sg;
                }
                if (live) *reinterpret_cast<floatx4*>(o.da2 + (int64_t)rm * NE + n * E + cc * 16 + 4 * g) = dlt;
                // dw1h += W_a2^T[:, n*E + cc*16 ..] . dlt   (a2T is [HE][NE])
#pragma unroll
                for (int mt = 0; mt < Mx::T1H; ++mt) {
                    floatx4 wa;
                    if constexpr (FAST)
                        wa = aT[cc][mt];
                    else
                        wa = ld4(Mon.a2T + (int64_t)(mt * 16 + col) * NE + n * E + cc * 16 + 4 * g);
                    dw1h[mt] = mfma_chunk(wa, dlt, dw1h[mt]);
                }
            }
            part += __shfl_xor(part, 16);
            part += __shfl_xor(part, 32);
            dq[n] = part;
        }
        // dwfh = W_f2^T . dwf -- MFMA needs every lane active, so it runs outside the store guard
        floatx4 dwfh[Mx::T1H];
#pragma unroll
        for (int mt = 0; mt < Mx::T1H; ++mt) {
            floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int cc = 0; cc < Mx::TE; ++cc)
                acc = mfma_chunk(ld4(Mon.f2T + (int64_t)(mt * 16 + col) * E + cc * 16 + 4 * g), dwf[cc], acc);
            dwfh[mt] = acc;
        }
        if (live) {
            float* d1 = o.d1 + (int64_t)rm * L1;
            float* la = o.l1act + (int64_t)rm * L1;
#pragma unroll
            for (int mt = 0; mt < Mx::T1H; ++mt) {  // w1h
                floatx4 v;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = l1[Mx::OW1 + mt][q] > 0.f ? dw1h[mt][q] : 0.f;
                *reinterpret_cast<floatx4*>(d1 + mt * 16 + 4 * g) = v;
            }
#pragma unroll
            for (int mt = 0; mt < Mx::T1H; ++mt) {  // wfh
                floatx4 acc = dwfh[mt];
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = l1[Mx::OWF + mt][q] > 0.f ? acc[q] : 0.f;
                *reinterpret_cast<floatx4*>(d1 + HE + mt * 16 + 4 * g) = acc;
            }
#pragma unroll
            for (int cc = 0; cc < Mx::TE; ++cc) {  // b1, vh
                *reinterpret_cast<floatx4*>(d1 + 2 * HE + cc * 16 + 4 * g) = dpre[cc];
                const floatx4 wv = ld4(Mon.v2p + cc * 16 + 4 * g);
                floatx4 v;
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = l1[Mx::OVH + cc][q] > 0.f ? dy * wv[q] : 0.f;
                *reinterpret_cast<floatx4*>(d1 + 2 * HE + E + cc * 16 + 4 * g) = v;
                *reinterpret_cast<floatx4*>(o.df2 + (int64_t)rm * E + cc * 16 + 4 * g) = dwf[cc];
            }
#pragma unroll
            for (int mt = 0; mt < Mx::L1T; ++mt) *reinterpret_cast<floatx4*>(la + mt * 16 + 4 * g) = l1[mt];
            if (g == 0) {
                o.dv2[rm] = dy;
                for (int k = 0; k < S; ++k) o.srow[(int64_t)rm * S + k] = s0[k];
            }
        }
    } else {
        for (int n = 0; n < N; ++n) dq[n] = dy;
    }
    // ---- dQ per agent row (t-major) and its one-hot expansion for dW2 ----
    if (live && g == 0) {
        for (int n = 0; n < N; ++n) {
            const int r = b * N + n;
            o.dq[(int64_t)t * c.R + r] = dq[n];
            const int a = (int)bt.actions[(bslot(bt, b) * bt.T1 + t) * N + n];
            o.d2[((int64_t)t * c.R + r) * c.A + a] = dq[n];
        }
    }
}

// ================================================================================================
// QMixer with one-layer hypernetworks (qmix.py:17-19) on one 16-row tile: hyper_w_1, hyper_w_final, hyper_b_1 and V.0
// all read the state row. The rows of m1 behind hyper_w_1's N E are l1 = [wf (pre-abs) | b1 | vh (post ReLU)];
// hyper_w_1's own N E outputs (up to 32 agents x 64 features per row) are never held: w1pre() computes one 16-feature
// chunk of one agent from the state when the forward and again when the backward needs it, as Mixer does.
template <int E>
struct Mixer1 {
    static constexpr int TE = E / 16, L1T = 3 * TE;
    static constexpr int OWF = 0, OB1 = TE, OVH = 2 * TE;

    __device__ static void layer1(const MixPtrs& M, const MixPack& mp, int S, const float* s, floatx4 (&l1)[L1T], int lane) {
        const int col = lane & 15, g = lane >> 4;
        const int r0 = mp.NE;
#pragma unroll
        for (int mt = 0; mt < L1T; ++mt) l1[mt] = ld4(M.mb1 + r0 + mt * 16 + 4 * g);
        for (int kc = 0; kc < mp.Sp / 16; ++kc) {
            const floatx4 sv = load_chunk(s, kc * 16 + 4 * g, S);
#pragma unroll
            for (int mt = 0; mt < L1T; ++mt)
                l1[mt] = mfma_chunk(ld4(M.m1 + (int64_t)(r0 + mt * 16 + col) * mp.Sp + kc * 16 + 4 * g), sv, l1[mt]);
        }
#pragma unroll
        for (int mt = OVH; mt < L1T; ++mt) {
#pragma unroll
            for (int q = 0; q < 4; ++q) l1[mt][q] = fmaxf(l1[mt][q], 0.f);
        }
    }

    // pre-abs hyper_w_1 output for agent n, chunk cc (features n*E + cc*16 ..), from the state row
    __device__ static floatx4 w1pre(const MixPtrs& M, const MixPack& mp, int S, const float* s, int n, int cc, int lane) {
        const int col = lane & 15, g = lane >> 4;
        floatx4 acc = ld4(M.mb1 + n * E + cc * 16 + 4 * g);
        const float* wrow = M.m1 + (int64_t)(n * E + cc * 16 + col) * mp.Sp + 4 * g;
        for (int kc = 0; kc < mp.Sp / 16; ++kc)
            acc = mfma_chunk(ld4(wrow + kc * 16), load_chunk(s, kc * 16 + 4 * g, S), acc);
        return acc;
    }

    __device__ static float vval(const MixPtrs& M, const floatx4 (&l1)[L1T], int lane) {
        const int col = lane & 15, g = lane >> 4;
        floatx4 acc = ld4(M.bv2p + 4 * g);
        const float* wrow = M.v2p + (int64_t)col * E + 4 * g;
#pragma unroll
        for (int kc = 0; kc < TE; ++kc) acc = mfma_chunk(ld4(wrow + kc * 16), l1[OVH + kc], acc);
        return __shfl(acc[0], col);  // feature 0 lives in lane group 0, reg 0
    }

    // forward: y per row (identical in the 4 lanes of a row); l1[OWF ..] are the pre-abs hyper_w_final outputs
    __device__ static float forward(const MixPtrs& M, const MixPack& mp, int S, int N, const float* s, const float* qrow,
                                    floatx4 (&l1)[L1T], floatx4 (&pre)[TE], floatx4 (&hid)[TE], int lane) {
        layer1(M, mp, S, s, l1, lane);
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) pre[cc] = l1[OB1 + cc];
        for (int n = 0; n < N; ++n) {
            const float qn = qrow[n];
#pragma unroll
            for (int cc = 0; cc < TE; ++cc) {
                const floatx4 wp = w1pre(M, mp, S, s, n, cc, lane);
#pragma unroll
                for (int q = 0; q < 4; ++q) pre[cc][q] += qn * fabsf(wp[q]);
            }
        }
        float part = 0.f;
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                hid[cc][q] = pre[cc][q] > 0.f ? pre[cc][q] : expm1f(pre[cc][q]);
                part += hid[cc][q] * fabsf(l1[OWF + cc][q]);
            }
        }
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        return part + vval(M, l1, lane);
    }
};

// mix_td_kernel for one-layer hypernetworks: the same two waves per 16-row tile (wave 0 the target mixer, wave 1 the
// online forward, TD and backward), the same loss partials and dq / d2 deltas. The hypernetworks have no hidden layer
// to carry a gradient back through: the weight-gradient deltas are the pre-abs hyper outputs' own (da2 [RM][N E] for
// hyper_w_1, df2 [RM][E] for hyper_w_final, d1 = [b1 | vh] [RM][2 E]), all against the state row; l1act [RM][E] keeps
// V's hidden activations for V.2.
template <int E, bool PER = false>
__global__ void __launch_bounds__(128) mix_td1_kernel(LCfg c, MlgBatch bt, MixPtrs Mon, MixPtrs Mtg, MixPack mp,
                                                     const float* __restrict__ mac, const float* __restrict__ tmac_,
                                                     const float* __restrict__ msum_p, MixOut o, Skip sk, PerIo pw) {
    using Mx = Mixer1<E>;
    __shared__ float tgt_sh[16];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    const int rm = blockIdx.x * 16 + col;
    const int Tm = c.T - 1;
    const bool valid = rm < c.RM;
    const int b = valid ? rm / Tm : 0, t = valid ? rm % Tm : 0;
    const int N = c.N, S = c.S, NE = N * E;
    // dead transitions as in mix_td_kernel: zeros for their Qs and state, nothing stored, exact zeros into the sums
    const bool live = valid && t < (int)sk.mlen[b];
    if (!__any(live)) {  // both waves of the tile alike
        if (wv == 1 && lane < 4) o.part[(int64_t)blockIdx.x * 4 + lane] = 0.f;
        return;
    }
    const bool tr = target_runs(c, sk);  // else the online buffers hold the target's bits
    const float* tmac = tr ? tmac_ : mac;
    const MixPtrs& Mt = tr ? Mtg : Mon;
    float cq[MAXN], tq[MAXN];
    for (int n = 0; n < N; ++n) cq[n] = tq[n] = 0.f;
    if (live) gather_q(c, bt, mac, tmac, b, t, cq, tq);
    const float m = live ? mask_at(bt, b, t) : 0.f;  // reference truncation: mlen <= t_eff - 1
    const float rwd = valid ? bt.reward[bslot(bt, b) * bt.T1 + t] : 0.f;
    const float term = valid ? (float)bt.terminated[bslot(bt, b) * bt.T1 + t] : 0.f;
    const float msum = msum_p[0];
    const float* s0 = live ? bt.state + (bslot(bt, b) * bt.T1 + t) * S : nullptr;
    const float* s1 = live ? bt.state + (bslot(bt, b) * bt.T1 + t + 1) * S : nullptr;
    float qtot = 0.f;
    floatx4 l1[Mx::L1T], pre[Mx::TE], hid[Mx::TE];
    if (wv == 0) {
        const float tv = Mx::forward(Mt, mp, S, N, s1, tq, l1, pre, hid, lane);
        if (g == 0) tgt_sh[col] = tv;
    } else {
        qtot = Mx::forward(Mon, mp, S, N, s0, cq, l1, pre, hid, lane);
    }
    __syncthreads();
    if (wv == 0) return;
    const float tgt = tgt_sh[col];
    const float y = rwd + c.gamma * (1.f - term) * tgt;  // q_learner.py:86
    const float mtd = (qtot - y) * m;                     // :89-95
    float dy = 2.f * mtd * m / msum;                      // d loss / d q_tot
    float wb = 1.f;
    if constexpr (PER) {  // the weighted loss; this row's share of its episode's error
        wb = pw.w[b];
        dy = 2.f * wb * mtd * m / msum;
        if (live && g == 0) pw.tdrow[rm] = fabsf(mtd);
    }
    {
        float p0 = g == 0 ? (PER ? wb * (mtd * mtd) : mtd * mtd) : 0.f, p1 = g == 0 ? fabsf(mtd) : 0.f;
        float p2 = g == 0 ? qtot * m : 0.f, p3 = g == 0 ? y * m : 0.f;
        p0 = row_sum16(p0);
        p1 = row_sum16(p1);
        p2 = row_sum16(p2);
        p3 = row_sum16(p3);
        if (lane == 0) {
            float* pp = o.part + (int64_t)blockIdx.x * 4;
            pp[0] = p0;
            pp[1] = p1;
            pp[2] = p2;
            pp[3] = p3;
        }
    }
    // ---- QMixer backward (autograd of qmix.py:41-59) ----
    floatx4 dpre[Mx::TE], dwf[Mx::TE];
#pragma unroll
    for (int cc = 0; cc < Mx::TE; ++cc) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float wf = l1[Mx::OWF + cc][q];
            const float dh = dy * fabsf(wf);
            const float sg = wf > 0.f ? 1.f : (wf < 0.f ? -1.f : 0.f);
            dwf[cc][q] = dy * hid[cc][q] * sg;
            dpre[cc][q] = pre[cc][q] > 0.f ? dh : dh * (hid[cc][q] + 1.f);
        }
    }
    float dq[MAXN];
    for (int n = 0; n < N; ++n) {
        float part = 0.f;
#pragma unroll
        for (int cc = 0; cc < Mx::TE; ++cc) {
            const floatx4 wp = Mx::w1pre(Mon, mp, S, s0, n, cc, lane);  // MFMA: every lane, outside the store guard
            floatx4 dlt;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                part += fabsf(wp[q]) * dpre[cc][q];
                const float sg = wp[q] > 0.f ? 1.f : (wp[q] < 0.f ? -1.f : 0.f);
                dlt[q] = cq[n] * dpre[cc][q] * sg;
            }
            if (live) *reinterpret_cast<floatx4*>(o.da2 + (int64_t)rm * NE + n * E + cc * 16 + 4 * g) = dlt;
        }
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        dq[n] = part;
    }
    if (live) {
        float* d1 = o.d1 + (int64_t)rm * 2 * E;
#pragma unroll
        for (int cc = 0; cc < Mx::TE; ++cc) {  // b1, vh, hyper_w_final, V's hidden activations
            *reinterpret_cast<floatx4*>(d1 + cc * 16 + 4 * g) = dpre[cc];
            const floatx4 wv2 = ld4(Mon.v2p + cc * 16 + 4 * g);
            floatx4 v;
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = l1[Mx::OVH + cc][q] > 0.f ? dy * wv2[q] : 0.f;
            *reinterpret_cast<floatx4*>(d1 + E + cc * 16 + 4 * g) = v;
            *reinterpret_cast<floatx4*>(o.df2 + (int64_t)rm * E + cc * 16 + 4 * g) = dwf[cc];
            *reinterpret_cast<floatx4*>(o.l1act + (int64_t)rm * E + cc * 16 + 4 * g) = l1[Mx::OVH + cc];
        }
        if (g == 0) {
            o.dv2[rm] = dy;
            for (int k = 0; k < S; ++k) o.srow[(int64_t)rm * S + k] = s0[k];
            for (int n = 0; n < N; ++n) {  // dQ per agent row (t-major) and its one-hot expansion for dW2
                const int r = b * N + n;
                o.dq[(int64_t)t * c.R + r] = dq[n];
                const int a = (int)bt.actions[(bslot(bt, b) * bt.T1 + t) * N + n];
                o.d2[((int64_t)t * c.R + r) * c.A + a] = dq[n];
            }
        }
    }
}

// IQL (mixer 0): no mixing, one TD error per (b, t, agent) against the agent's own target, the mask expanded over the
// agents (msum_p[0] * N = mask_elems divides the loss; stored to msum_p[2], which finish_kernel then takes as its mask
// sum, so every statistic's denominator, stats[5], stats[6] and trained_steps follow the expanded mask). One wave per
// 16 (b, t) rows, as the mixer kernels' tiles:
// lane (col, g) takes row col's agents g, g + 4, ... in order; the four groups of a row and then the 16 rows are summed
// in a fixed order into the tile's four partials. Writes the same sparse dq / d2 deltas as the mixer kernels.
template <bool PER = false>
__global__ void __launch_bounds__(64) iql_td_kernel(LCfg c, MlgBatch bt, const float* __restrict__ mac,
                                                   const float* __restrict__ tmac_, float* __restrict__ msum_p,
                                                   MixOut o, Skip sk, PerIo pw) {
    const int lane = threadIdx.x, col = lane & 15, g = lane >> 4;
    const float melems = msum_p[0] * (float)c.N;  // sum of the expanded mask (q_learner.py:92)
    if (blockIdx.x == 0 && lane == 0) msum_p[2] = melems;  // finish_kernel's mask sum for this call (msum[2] is free)
    const int rm = blockIdx.x * 16 + col;
    const int Tm = c.T - 1;
    const bool valid = rm < c.RM;
    const int b = valid ? rm / Tm : 0, t = valid ? rm % Tm : 0;
    const bool live = valid && t < (int)sk.mlen[b];  // dead transitions: mask 0, exact zeros, nothing stored
    if (!__any(live)) {
        if (lane < 4) o.part[(int64_t)blockIdx.x * 4 + lane] = 0.f;
        return;
    }
    const float* tmac = target_runs(c, sk) ? tmac_ : mac;  // else the online buffer holds the target's bits
    float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
    if (live) {
        const float m = mask_at(bt, b, t);
        const float rwd = bt.reward[bslot(bt, b) * bt.T1 + t];
        const float term = (float)bt.terminated[bslot(bt, b) * bt.T1 + t];
        float wb = 1.f;
        if constexpr (PER) wb = pw.w[b];
        for (int n = g; n < c.N; n += 4) {
            int a;
            float cq, tq;
            gather_q1(c, bt, mac, tmac, b, t, n, a, cq, tq);
            const float y = rwd + c.gamma * (1.f - term) * tq;  // q_learner.py:86
            const float mtd = (cq - y) * m;                      // :89-95
            float dy = 2.f * mtd * m / melems;                   // d loss / d Q_chosen[b, t, n]
            if constexpr (PER) dy = 2.f * wb * mtd * m / melems;
            p0 += PER ? wb * (mtd * mtd) : mtd * mtd;
            p1 += fabsf(mtd);
            p2 += cq * m;
            p3 += y * m;
            const int64_t row = (int64_t)t * c.R + b * c.N + n;
            o.dq[row] = dy;
            o.d2[row * c.A + a] = dy;
        }
    }
    float p[4] = {p0, p1, p2, p3};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        p[k] += __shfl_xor(p[k], 16);
        p[k] += __shfl_xor(p[k], 32);
        if constexpr (PER) {  // the row's |td| over its agents: groups 0..3 in this fixed order
            if (k == 1 && live && g == 0) pw.tdrow[rm] = p[1];
        }
        p[k] = row_sum16(p[k]);
    }
    if (lane == 0) {
        float* pp = o.part + (int64_t)blockIdx.x * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) pp[k] = p[k];
    }
}

// ================================================================================================
// Split mixer (default for the FAST shapes): the QMixer's hypernetworks read only the state (qmix.py:41-52: hyper_w_1,
// hyper_b_1, hyper_w_final, V), not the agent network, so their forward -- about two thirds of mix_td's matrix work --
// runs beside the agent recurrence, in the same launch (rec4_mixpre_kernel) on the CUs the recurrence leaves idle. Per (b, t) row it stores the
// pre-abs hyper_w_1 outputs of every agent, the pre-abs hyper_w_final outputs, hyper_b_1 and V: online on s_t, target
// on s_{t+1}; the online net also stores its layer-1 activations and the state row for the weight gradients.
// mix_td2_kernel then gathers the Qs, mixes (MixerPF::mix), forms the TD error and runs the mixer backward exactly as
// mix_td_kernel does. Same operations in the same order: bit-identical to mix_td_kernel<.., true>.
struct HypOut {
    float *on, *tg;  // [RM][hs]: w1p [N*E] | wfp [E] | b1 [E] | v (padded to 4)
    float *la, *srow;
    int hs;
};

// One 16-row tile by a pair of waves: wv 0 the target net on s_{t+1}, wv 1 the online net on s_t.
template <int HE, int E>
__device__ __forceinline__ void mix_pre_tile(const LCfg& c, const MlgBatch& bt, const MixPtrs& Mon, const MixPtrs& Mtg,
                                             const MixPack& mp, const HypOut& o, const Skip& sk, int tile, int wv,
                                             int lane) {
    using Mx = Mixer<HE, E>;
    using MP = MixerPF<HE, E, 4, MIXPF_N>;
    const int col = lane & 15, g = lane >> 4;
    const bool tgt = wv == 0;
    const int rm = tile * 16 + col;
    const int Tm = c.T - 1;
    const bool valid = rm < c.RM;
    const int b = valid ? rm / Tm : 0, t = valid ? rm % Tm : 0;
    const int N = c.N, S = c.S, NE = N * E, L1 = 2 * HE + 2 * E;
    {  // Which rows of the tile does mix_td2 read? (a wave that has any stores all of its tile's rows)
        //   online: s_t of a live transition (t < mlen) and, as the target's input while the target net is a copy of the
        //           online one, s_{t+1} of the episode's last live transition: t <= mlen
        //   target: s_{t+1} of the live transitions; while it is a copy, only those whose t + 1 has no online row
        //           (t = T - 2: the online rows end there)
        const int ml = valid ? (int)sk.mlen[b] : 0;
        const bool need = valid && (tgt ? t < ml && (t == Tm - 1 || target_runs(c, sk)) : t <= ml);
        if (!__any(need)) return;
    }
    const float* s = valid ? bt.state + (bslot(bt, b) * bt.T1 + t + (tgt ? 1 : 0)) * S : nullptr;
    floatx4 l1[Mx::L1T], w1p[MIXPF_N][Mx::TE], wfp[Mx::TE];
    float v;
    MP::hyper(tgt ? Mtg : Mon, mp, S, N, s, l1, w1p, wfp, v, lane);
    if (!valid) return;
    float* h = (tgt ? o.tg : o.on) + (int64_t)rm * o.hs;
#pragma unroll
    for (int n = 0; n < MIXPF_N; ++n) {
        if (n >= N) break;
#pragma unroll
        for (int cc = 0; cc < Mx::TE; ++cc) *reinterpret_cast<floatx4*>(h + n * E + cc * 16 + 4 * g) = w1p[n][cc];
    }
#pragma unroll
    for (int cc = 0; cc < Mx::TE; ++cc) {
        *reinterpret_cast<floatx4*>(h + NE + cc * 16 + 4 * g) = wfp[cc];
        *reinterpret_cast<floatx4*>(h + NE + E + cc * 16 + 4 * g) = l1[Mx::OB1 + cc];
    }
    if (g == 0) h[NE + 2 * E] = v;
    if (!tgt) {
        float* la = o.la + (int64_t)rm * L1;
#pragma unroll
        for (int mt = 0; mt < Mx::L1T; ++mt) *reinterpret_cast<floatx4*>(la + mt * 16 + 4 * g) = l1[mt];
        if (g == 0)
            for (int k = 0; k < S; ++k) o.srow[(int64_t)rm * S + k] = s[k];
    }
}

// The agent recurrence (agent_rec4_kernel, blocks < 2 * ntiles4) and the mixer's hypernetwork forward (mix_pre_tile,
// blockDim / 128 tiles per block after them) in one launch: the recurrence occupies (R / 4) * 2 CUs for its whole
// sequential T loop, the hypernet tiles run on the idle ones, with no cross-stream fork / join.
template <int H>
__global__ void __launch_bounds__(512) rec4_mixpre_kernel(LCfg c, AgentLayout L, const float* __restrict__ Pon,
                                                          const float* __restrict__ Ptg, const float* __restrict__ gi_on,
                                                          const float* __restrict__ gi_tg, float* __restrict__ hs_on,
                                                          float* __restrict__ hs_tg, float* __restrict__ ws_gr,
                                                          float* __restrict__ ws_gz, float* __restrict__ ws_gn,
                                                          float* __restrict__ ws_ghn, Skip sk,
                                                          MlgBatch bt, MixPtrs Mon, MixPtrs Mtg, MixPack mp, HypOut o) {
    const int nrec = 2 * ((c.R + 3) / 4);
    if ((int)blockIdx.x < nrec) {
        agent_rec4_body<H>(c, L, Pon, Ptg, gi_on, gi_tg, hs_on, hs_tg, ws_gr, ws_gz, ws_gn, ws_ghn, sk, blockIdx.x, c.R);
        return;
    }
    const int w = threadIdx.x >> 6, per = blockDim.x / 128;
    const int tile = ((int)blockIdx.x - nrec) * per + (w >> 1);
    if (tile * 16 >= c.RM) return;  // whole pair of waves past the last tile (block-uniform per wave pair)
    mix_pre_tile<64, 32>(c, bt, Mon, Mtg, mp, o, sk, tile, w & 1, threadIdx.x & 63);
}

template <int HE, int E, bool PER = false>
__global__ void __launch_bounds__(128) mix_td2_kernel(LCfg c, MlgBatch bt, MixPtrs Mon, const float* __restrict__ mac,
                                                      const float* __restrict__ tmac_, const float* __restrict__ msum_p,
                                                      HypOut hy, MixOut o, Skip sk, PerIo pw) {
    using Mx = Mixer<HE, E>;
    using MP = MixerPF<HE, E, 4, MIXPF_N>;
    constexpr int TE = Mx::TE, T1H = Mx::T1H;
    __shared__ float tgt_sh[16];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 15, g = lane >> 4;
    const int rm = blockIdx.x * 16 + col;
    const int Tm = c.T - 1;
    const bool valid = rm < c.RM;
    const int b = valid ? rm / Tm : 0, t = valid ? rm % Tm : 0;
    const int N = c.N, NE = N * E, L1 = 2 * HE + 2 * E;
    // dead transitions as in mix_td_kernel: zeros for their Qs, nothing stored, exact zeros into the tile's sums
    const bool live = valid && t < (int)sk.mlen[b];
    const uint64_t lv = __ballot(live);
    if (!lv) {  // both waves of the tile alike
        if (wv == 1 && lane < 4) o.part[(int64_t)blockIdx.x * 4 + lane] = 0.f;
        return;
    }
    const bool tr = target_runs(c, sk);  // else the online buffers hold the target's bits
    const float* tmac = tr ? tmac_ : mac;
    // this lane's hypernet outputs. Online (wave 1): its own row; mix_pre_tile stored every row of a tile that has a
    // live one, and row 0 (rows past RM) is always among them. Target (wave 0): its own row of hy.tg, or while the
    // target net is a copy of the online one the online outputs on s_{t+1} = row rm + 1 (t = T - 2 has none: hy.tg,
    // see mix_pre_tile); a dead lane takes the row of the tile's first live lane, which is there and finite.
    const float* h;
    if (wv == 0) {
        int use_on = (!tr && t + 1 < Tm) ? 1 : 0, row = use_on ? rm + 1 : rm;
        const int first = __builtin_ctzll(lv);
        const int f_on = __shfl(use_on, first), f_row = __shfl(row, first);
        if (!live) {
            use_on = f_on;
            row = f_row;
        }
        h = (use_on ? hy.on : hy.tg) + (int64_t)row * hy.hs;
    } else {
        h = hy.on + (int64_t)(valid ? rm : 0) * hy.hs;
    }
    floatx4 w1c[MIXPF_N][TE], wfp[TE], b1[TE];
#pragma unroll
    for (int n = 0; n < MIXPF_N; ++n) {
        if (n >= N) break;
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) w1c[n][cc] = ld4(h + n * E + cc * 16 + 4 * g);
    }
#pragma unroll
    for (int cc = 0; cc < TE; ++cc) {
        wfp[cc] = ld4(h + NE + cc * 16 + 4 * g);
        b1[cc] = ld4(h + NE + E + cc * 16 + 4 * g);
    }
    const float vv = h[NE + 2 * E];
    // operands of the backward that depend on nothing computed here, requested now so that their L2 / HBM round
    // trips overlap the gather and the mixing (wave 1 only: wave 0 leaves after the target mix): agent 0's W_a2^T
    // block, W_f2^T, V's output row and this row's layer-1 activations (stored by mix_pre_tile)
    const float* la = hy.la + (int64_t)(valid ? rm : 0) * L1;
    floatx4 aTb[2][TE][T1H], f2w[T1H][TE], wvb[TE], lab[T1H * 2 + TE];
    auto load_aT = [&](int n, floatx4 (&d)[TE][T1H]) {
#pragma unroll
        for (int cc = 0; cc < TE; ++cc)
#pragma unroll
            for (int mt = 0; mt < T1H; ++mt) d[cc][mt] = ld4(Mon.a2T + (int64_t)(mt * 16 + col) * NE + n * E + cc * 16 + 4 * g);
    };
    if (wv == 1) {
        load_aT(0, aTb[0]);
#pragma unroll
        for (int mt = 0; mt < T1H; ++mt)
#pragma unroll
            for (int cc = 0; cc < TE; ++cc) f2w[mt][cc] = ld4(Mon.f2T + (int64_t)(mt * 16 + col) * E + cc * 16 + 4 * g);
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) wvb[cc] = ld4(Mon.v2p + cc * 16 + 4 * g);
#pragma unroll
        for (int mt = 0; mt < T1H; ++mt) {
            lab[mt] = ld4(la + (Mx::OW1 + mt) * 16 + 4 * g);
            lab[T1H + mt] = ld4(la + (Mx::OWF + mt) * 16 + 4 * g);
        }
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) lab[2 * T1H + cc] = ld4(la + (Mx::OVH + cc) * 16 + 4 * g);
    }
    float cq[MAXN], tq[MAXN];
    for (int n = 0; n < N; ++n) cq[n] = tq[n] = 0.f;
    gather_q_rows<MIXPF_A>(c, bt, mac, tmac, b, t, live, g, cq, tq);
    floatx4 pre[TE], hid[TE];
    if (wv == 0) {
        const float tv = MP::mix(N, tq, b1, w1c, wfp, vv, pre, hid);
        if (g == 0) tgt_sh[col] = tv;
    }
    const float m = live ? mask_at(bt, b, t) : 0.f;  // reference truncation: mlen <= t_eff - 1
    const float rwd = valid ? bt.reward[bslot(bt, b) * bt.T1 + t] : 0.f;
    const float term = valid ? (float)bt.terminated[bslot(bt, b) * bt.T1 + t] : 0.f;
    const float msum = msum_p[0];
    float qtot = 0.f;
    if (wv == 1) qtot = MP::mix(N, cq, b1, w1c, wfp, vv, pre, hid);
    __syncthreads();
    if (wv == 0) return;
    const float tgt = tgt_sh[col];
    const float y = rwd + c.gamma * (1.f - term) * tgt;  // q_learner.py:86
    const float mtd = (qtot - y) * m;                     // :89-95
    float dy = 2.f * mtd * m / msum;                      // d loss / d q_tot
    float wb = 1.f;
    if constexpr (PER) {  // the weighted loss; this row's share of its episode's error
        wb = pw.w[b];
        dy = 2.f * wb * mtd * m / msum;
        if (live && g == 0) pw.tdrow[rm] = fabsf(mtd);
    }
    {
        float p0 = g == 0 ? (PER ? wb * (mtd * mtd) : mtd * mtd) : 0.f, p1 = g == 0 ? fabsf(mtd) : 0.f;
        float p2 = g == 0 ? qtot * m : 0.f, p3 = g == 0 ? y * m : 0.f;
        p0 = row_sum16(p0);
        p1 = row_sum16(p1);
        p2 = row_sum16(p2);
        p3 = row_sum16(p3);
        if (lane == 0) {
            float* pp = o.part + (int64_t)blockIdx.x * 4;
            pp[0] = p0;
            pp[1] = p1;
            pp[2] = p2;
            pp[3] = p3;
        }
    }
    // ---- QMixer backward (autograd of qmix.py:41-59), as mix_td_kernel ----
    floatx4 dpre[TE], dwf[TE];
#pragma unroll
    for (int cc = 0; cc < TE; ++cc) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float dh = dy * fabsf(wfp[cc][q]);
            const float sg = wfp[cc][q] > 0.f ? 1.f : (wfp[cc][q] < 0.f ? -1.f : 0.f);
            dwf[cc][q] = dy * hid[cc][q] * sg;
            dpre[cc][q] = pre[cc][q] > 0.f ? dh : dh * (hid[cc][q] + 1.f);
        }
    }
    floatx4 dw1h[T1H];
#pragma unroll
    for (int mt = 0; mt < T1H; ++mt) dw1h[mt] = floatx4{0.f, 0.f, 0.f, 0.f};
    float dq[MAXN];
#pragma unroll
    for (int n = 0; n < MIXPF_N; ++n) {  // N <= MIXPF_N (the FAST shapes): static ping-pong buffers
        if (n >= N) break;
        if (n + 1 < MIXPF_N && n + 1 < N) load_aT(n + 1, aTb[(n + 1) & 1]);
        const floatx4(&aT)[TE][T1H] = aTb[n & 1];
        float part = 0.f;
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) {
            const floatx4 wp = w1c[n][cc];
            floatx4 dlt;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                part += fabsf(wp[q]) * dpre[cc][q];
                const float sg = wp[q] > 0.f ? 1.f : (wp[q] < 0.f ? -1.f : 0.f);
                dlt[q] = cq[n] * dpre[cc][q] * sg;
            }
            if (live) *reinterpret_cast<floatx4*>(o.da2 + (int64_t)rm * NE + n * E + cc * 16 + 4 * g) = dlt;
#pragma unroll
            for (int mt = 0; mt < T1H; ++mt) dw1h[mt] = mfma_chunk(aT[cc][mt], dlt, dw1h[mt]);
        }
        part += __shfl_xor(part, 16);
        part += __shfl_xor(part, 32);
        dq[n] = part;
    }
    floatx4 dwfh[T1H];
#pragma unroll
    for (int mt = 0; mt < T1H; ++mt) {
        floatx4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) acc = mfma_chunk(f2w[mt][cc], dwf[cc], acc);
        dwfh[mt] = acc;
    }
    if (live) {
        // layer-1 activations (stored by mix_pre_tile, loaded above) for the ReLU masks
        float* d1 = o.d1 + (int64_t)rm * L1;
#pragma unroll
        for (int mt = 0; mt < T1H; ++mt) {  // w1h
            const floatx4 l = lab[mt];
            floatx4 v;
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = l[q] > 0.f ? dw1h[mt][q] : 0.f;
            *reinterpret_cast<floatx4*>(d1 + mt * 16 + 4 * g) = v;
        }
#pragma unroll
        for (int mt = 0; mt < T1H; ++mt) {  // wfh
            const floatx4 l = lab[T1H + mt];
            floatx4 acc = dwfh[mt];
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[q] = l[q] > 0.f ? acc[q] : 0.f;
            *reinterpret_cast<floatx4*>(d1 + HE + mt * 16 + 4 * g) = acc;
        }
#pragma unroll
        for (int cc = 0; cc < TE; ++cc) {  // b1, vh
            *reinterpret_cast<floatx4*>(d1 + 2 * HE + cc * 16 + 4 * g) = dpre[cc];
            const floatx4 wv = wvb[cc];
            const floatx4 l = lab[2 * T1H + cc];
            floatx4 v;
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = l[q] > 0.f ? dy * wv[q] : 0.f;
            *reinterpret_cast<floatx4*>(d1 + 2 * HE + E + cc * 16 + 4 * g) = v;
            *reinterpret_cast<floatx4*>(o.df2 + (int64_t)rm * E + cc * 16 + 4 * g) = dwf[cc];
        }
        if (g == 0) o.dv2[rm] = dy;
    }
    if (live && g == 0) {  // dQ per agent row (t-major) and its one-hot expansion for dW2 (d2 zeroed by prep_kernel:
                            // whole-row writes here measured 3.7 us slower, and the zeroing is off prep's critical path)
        for (int n = 0; n < N; ++n) {
            const int r = b * N + n;
            o.dq[(int64_t)t * c.R + r] = dq[n];
            const int a = (int)bt.actions[(bslot(bt, b) * bt.T1 + t) * N + n];
            o.d2[((int64_t)t * c.R + r) * c.A + a] = dq[n];
        }
    }
}

// ================================================================================================
// reverse-time GRU backward: dh_{t-1} = dh * z + W_hh^T dGH.  dX = W_ih^T dGI does not feed the recurrence:
// agent_dx_kernel.
// The backward recurrence on 4-row tiles (v_mfma_f32_4x4x1_16b_f32, as agent_rec4_kernel). Wave w owns hidden
// features 16w..16w+15; block b = 4kq + fg accumulates W_hh^T dGH for features 16w + 4fg + i over the K quarter
// kq (48 of the 3H gate rows, W_hh columns in VGPRs). The four quarter partials are summed across the wave's
// 16-lane rows with a transposing reduction (rows_sum_transpose4): lane (row kq, fg, j) ends up owning feature
// 16w + 4fg + kq of row j, so all 64 lanes run the elementwise GRU backward, one (feature, row) each.
// grid (ntiles4), H/16 waves.
// DX (distinct networks): grid (ntiles4 of one instance, N), y = ag; dQ of instance row r = b is the mixer's row b N + ag.
template <int H, bool DX = false>
__global__ void __launch_bounds__(512) agent_bwd4_kernel(LCfg c, MlgBatch bt, AgentLayout L, const float* __restrict__ P,
                                                         const float* __restrict__ ws_hs, const float* __restrict__ ws_gr,
                                                         const float* __restrict__ ws_gz, const float* __restrict__ ws_gn,
                                                         const float* __restrict__ ws_ghn, const float* __restrict__ dqv,
                                                         float* __restrict__ dgi, float* __restrict__ dgh, Skip sk) {
    LStamps lst;
    lst.init();
    if constexpr (DX) {
        const int ag = blockIdx.y;
        const DxView v = dx_view(c, L, ag);
        P += v.p;
        const int r = blockIdx.x * 4 + ((threadIdx.x & 63) & 3);
        const int b = r < c.B ? r : 0;
        const mlg::Gru4Bwd a{c.B, c.T, c.A, c.N, P + L.whh, P + L.w2, ws_hs + v.hs, ws_gr + v.h, ws_gz + v.h, ws_gn + v.h,
                             ws_ghn + v.h, dqv + ag, bt.actions, dgi + v.g3, dgh + v.g3, 0, c.N};
        mlg::gru4_bwd<H>(a, blockIdx.x, tile_steps(sk, blockIdx.x >> 2), bslot(bt, b) * bt.T1 * c.N + ag, lst);
        lst.flush(1);
    } else {
        const int r = blockIdx.x * 4 + ((threadIdx.x & 63) & 3);
        const bool valid = r < c.R;
        const int b = valid ? r / c.N : 0, n = valid ? r % c.N : 0;
        const mlg::Gru4Bwd a{c.R, c.T, c.A, c.N, P + L.whh, P + L.w2, ws_hs, ws_gr, ws_gz, ws_gn, ws_ghn, dqv,
                             bt.actions, dgi, dgh, 0};  // no zeroed tail: the weight gradients skip those rows
        mlg::gru4_bwd<H>(a, blockIdx.x, tile_steps(sk, blockIdx.x >> 2), bslot(bt, b) * bt.T1 * c.N + n, lst);
        lst.flush(1);
    }
}

// The reverse recurrence (blocks < nbwd, H = 64: 4 waves each) and, as the launch's remaining workgroups, the weight
// gradients whose deltas are final after the mixer kernel (fc2 and the mixer's jobs: table view JA). The
// recurrence keeps 40 CUs busy for its 101 sequential steps; the wgrad workgroups fill the others, with no second
// stream and no events (each event record costs a few us of queue time). Same per-job arithmetic as the separate
// launches.
template <int H>
__global__ void __launch_bounds__(256, 2) bwd4_wgrad_kernel(LCfg c, MlgBatch bt, AgentLayout L, const float* __restrict__ P,
                                                         const float* __restrict__ ws_hs, const float* __restrict__ ws_gr,
                                                         const float* __restrict__ ws_gz, const float* __restrict__ ws_gn,
                                                         const float* __restrict__ ws_ghn, const float* __restrict__ dqv,
                                                         float* __restrict__ dgi, float* __restrict__ dgh, Skip sk,
                                                         WJobs JA, float* __restrict__ slab, int nbwd) {
    if ((int)blockIdx.x >= nbwd) {
        mlg::wgrad_block_body<16>(JA, slab, (int)blockIdx.x - nbwd);
        return;
    }
    LStamps lst;
    lst.init();
    const int r = blockIdx.x * 4 + ((threadIdx.x & 63) & 3);
    const bool valid = r < c.R;
    const int b = valid ? r / c.N : 0, n = valid ? r % c.N : 0;
    const mlg::Gru4Bwd a{c.R, c.T, c.A, c.N, P + L.whh, P + L.w2, ws_hs, ws_gr, ws_gz, ws_gn, ws_ghn, dqv,
                         bt.actions, dgi, dgh, 0};  // no zeroed tail: the weight gradients skip those rows
    mlg::gru4_bwd<H>(a, blockIdx.x, tile_steps(sk, blockIdx.x >> 2), bslot(bt, b) * bt.T1 * c.N + n, lst);
    lst.flush(1);
}

// dA = (W_ih^T dGI) * (x > 0) for every (t, row): grid (ntiles, T), HC waves (wave = feature chunk).
// DX (distinct networks): grid (ntiles, T, N), z = ag.
template <int H, bool DX = false>
__global__ void __launch_bounds__(512) agent_dx_kernel(LCfg c, const float* __restrict__ wihT,
                                                       const float* __restrict__ ws_x, const float* __restrict__ dgi,
                                                       float* __restrict__ da, Skip sk) {
    const int tile = blockIdx.x, t = blockIdx.y;
    if (t >= tile_steps(sk, tile)) return;  // the fc1 weight gradient skips the block's rows
    if constexpr (DX) {
        const int64_t TB = (int64_t)c.T * c.B, ag = blockIdx.z;
        wihT += ag * 3 * H * H, ws_x += ag * TB * H, dgi += ag * TB * 3 * H, da += ag * TB * H;
    }
    const int R = DX ? c.B : c.R;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int col = lane & 15, g = lane >> 4;
    const int r = tile * 16 + col;
    const bool valid = r < R;
    const int64_t row = (int64_t)t * R + (valid ? r : 0);
    const float* wrow = wihT + (int64_t)(w * 16 + col) * 3 * H + 4 * g;
    const float* grow = dgi + row * 3 * H + 4 * g;
    const int64_t o = row * H + w * 16 + 4 * g;
    const floatx4 xv = ld4(ws_x + o);  // the ReLU mask, requested with the operands (row 0 for padding lanes)
    floatx4 dx = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc = 0; kc < 3 * H / 16; ++kc) dx = mfma_chunk(ld4(wrow + kc * 16), ld4(grow + kc * 16), dx);
    if (valid) {
#pragma unroll
        for (int q = 0; q < 4; ++q) dx[q] = xv[q] > 0.f ? dx[q] : 0.f;
        *reinterpret_cast<floatx4*>(da + o) = dx;
    }
}

// ================================================================================================
// Prioritized replay: td_abs[b] = sum_t tdrow[b (T - 1) + t] / (div sum_t mask(b, t)) over the episode's live
// transitions t < mlen[b] (the rows the PER form of the TD kernel stored in this call), div = N for IQL (the mask
// expanded over the agents), else 1; 0 for an episode with no masked step. One wave per episode: lane l adds the steps
// l, l + 64, ... in ascending order, then the 64 partial sums meet in a butterfly -- a fixed order, no atomics.
__global__ void __launch_bounds__(64) per_reduce_kernel(LCfg c, MlgBatch bt, const float* __restrict__ tdrow, Skip sk,
                                                       float div, float* __restrict__ td_abs) {
    const int b = blockIdx.x, lane = threadIdx.x, Tm = c.T - 1;
    const int n = min((int)sk.mlen[b], Tm);
    float e = 0.f, m = 0.f;
    for (int t = lane; t < n; t += 64) {
        e += tdrow[(int64_t)b * Tm + t];
        m += mask_at(bt, b, t);
    }
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        e += __shfl_xor(e, k);
        m += __shfl_xor(m, k);
    }
    if (lane == 0) td_abs[b] = m > 0.f ? e / (m * div) : 0.f;
}

// ================================================================================================
// clip_grad_norm_ + RMSprop over all parameters (grid-wide; every block derives the same norm from the
// per-block partials in a fixed order), loss/stat reduction in block 0, which also reports the planned forward blocks
// (stats[7]) and clears Skip::flag for the next call.
__global__ void __launch_bounds__(1024) finish_kernel(const float* __restrict__ part, int n_part,
                                                      const float* __restrict__ msum_p, float* __restrict__ params,
                                                      float* __restrict__ grads, float* __restrict__ sq, int64_t n_params,
                                                      float lr, float alpha, float eps, float max_norm, int N,
                                                      float* __restrict__ stats, const float* __restrict__ nrm_part,
                                                      int n_nrm, float* __restrict__ tsync, double* __restrict__ trained,
                                                      Skip sk, unsigned* __restrict__ flag, int ntiles, int full,
                                                      int nets) {  // distinct networks: N instances ran the tiles, and
                                                                   // trained[0 .. N - 1] count (1 otherwise)
    __shared__ float red[1024];
    const int tid = threadIdx.x;
    // the planned forward blocks (stats[7]: exact integers, any order) and the flag, requested ahead of the step
    float blocks = 0.f;
    unsigned fl = 0u;
    if (blockIdx.x == 0 && tid < 64) {
        for (int k = tid; k < ntiles; k += 64) blocks += sk.l16[k];
        fl = *flag;
    }
    // target update due after this step (q_learner.py:127-128): tsync
    const float norm = mlg::clip_rmsprop_step(params, grads, sq, n_params, nrm_part, n_nrm, lr, alpha, eps, max_norm,
                                              tsync, red);
    // the four stat sums on blocks 0..3 (one each, same order as one block doing all four: bit-identical), so no
    // block runs four block reductions after its parameter slice
    const float ms = msum_p[0];
    for (int k = blockIdx.x; k < 4; k += gridDim.x) {
        float v = 0.f;
        for (int j = tid; j < n_part; j += blockDim.x) v += part[(int64_t)j * 4 + k];
        const float sk = block_sum_1024(v, red);
        if (tid == 0) {
            if (k == 0) stats[0] = sk / ms;
            else if (k == 1) stats[2] = sk / ms;
            else stats[k + 1] = sk / (ms * N);  // k = 2, 3: stats[3], stats[4] (per agent)
        }
    }
    if (blockIdx.x == 0 && tid < 64) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) blocks += __shfl_xor(blocks, m);
    }
    if (blockIdx.x == 0 && tid == 0) {
        stats[1] = norm;
        stats[5] = ms;
        stats[6] = ms;
        blocks *= (float)nets;
        stats[7] = (full || fl == 1u) ? 2.f * blocks : blocks;  // forward (16-row tile, t, net) blocks of this call
        *flag = 0u;  // the next call's prep_kernel stores 1 where its target differs
        if (trained)
            for (int k = 0; k < nets; ++k) trained[k] += (double)ms;  // Agent.trained_steps (q_learner.py:104)
    }
}

// ================================================================================================
// host side
struct Plan {
    LCfg c;
    AgentLayout L;
    AgentOffs ao;
    MixOffs mo;
    MixPack mp;
    WsLayout w;
    int64_t n_agent, n_mixer;
    int layers;  // qmix hypernet_layers (1 or 2)
    int per;     // MlgLearnerCfg.per: the PER forms of the TD kernels + per_reduce_kernel
};

int check_cfg(const MlgLearnerCfg* c) {
    MLG_REQUIRE(c != nullptr, "null learner cfg");
    MLG_REQUIRE(c->H == 32 || c->H == 64 || c->H == 128, "rnn_hidden_dim=%d unsupported (32/64/128)", c->H);
    MLG_REQUIRE(c->B >= 1 && c->T >= 2 && c->N >= 1 && c->N <= MAXN && c->A >= 1, "learner: bad sizes B=%d T=%d N=%d",
                c->B, c->T, c->N);
    MLG_REQUIRE(c->A <= MLG_BWD_MAXA, "learner: n_actions=%d > %d unsupported", c->A, MLG_BWD_MAXA);
    MLG_REQUIRE((int64_t)c->T * c->B * c->N * 3 * c->H < (int64_t)1 << 29,
                "learner: T*B*N*3H=%lld floats exceeds the 2 GB buffer-store range",
                (long long)c->T * c->B * c->N * 3 * c->H);
    MLG_REQUIRE(c->mixer >= 0 && c->mixer <= 2, "learner: mixer=%d unsupported (0 none, 1 vdn, 2 qmix)", c->mixer);
    MLG_REQUIRE(c->agent == 0 || c->agent == 1, "learner: agent=%d unsupported (0 rnn: DRQN, 1 dqn: feed-forward)", c->agent);
    MLG_REQUIRE(c->distinct == 0 || c->distinct == 1, "learner: distinct=%d unsupported (0 shared agent, 1 one DRQN per slot)",
                c->distinct);
    if (c->distinct) {
        MLG_REQUIRE(c->agent == 0, "learner: agent=%d with distinct=1 unsupported (distinct networks are DRQNs, agent=0)",
                    c->agent);
        MLG_REQUIRE(!c->obs_agent_id, "learner: obs_agent_id=%d with distinct=1 unsupported (a slot's network is its id)",
                    c->obs_agent_id);
    }
    MLG_REQUIRE(c->per == 0 || c->per == 1, "learner: per=%d unsupported (0 uniform replay, 1 prioritized replay)", c->per);
    if (c->mixer == 2) {
        MLG_REQUIRE(c->hypernet_layers == 1 || c->hypernet_layers == 2, "learner: qmix hypernet_layers=%d unsupported (1, 2)",
                    c->hypernet_layers);
        MLG_REQUIRE(c->E == 16 || c->E == 32 || c->E == 64, "learner: qmix mixing_embed_dim=%d unsupported (16, 32, 64)",
                    c->E);
        MLG_REQUIRE(c->hypernet_layers == 1 || c->HE == 32 || c->HE == 64 || c->HE == 128,
                    "learner: qmix hypernet_embed=%d unsupported (32, 64, 128)", c->HE);
    }
    return 0;
}

Plan make_plan(const MlgLearnerCfg* cfg, int T1) {
    Plan p;
    LCfg& c = p.c;
    c.B = cfg->B;
    c.T = cfg->T;
    c.T1 = T1;
    c.N = cfg->N;
    c.A = cfg->A;
    c.Ap = (cfg->A + 15) / 16 * 16;
    c.d_obs = cfg->d_obs;
    c.d_in = cfg->d_obs + (cfg->obs_last_action ? cfg->A : 0) + (cfg->obs_agent_id ? cfg->N : 0);
    c.H = cfg->H;
    c.S = cfg->S;
    c.E = cfg->E;
    c.HE = cfg->HE;
    c.mixer = cfg->mixer;
    c.double_q = cfg->double_q;
    c.last_action = cfg->obs_last_action;
    c.agent_id = cfg->obs_agent_id;
    c.R = cfg->B * cfg->N;
    c.RM = cfg->B * (cfg->T - 1);
    c.gamma = cfg->gamma;
    c.full = getenv("MLG_LEARNER_FULL") != nullptr;  // read per call, so a test can set it
    c.ff = cfg->agent == 1;
    c.dx = cfg->distinct == 1;
    p.layers = cfg->mixer == 2 ? cfg->hypernet_layers : 2;
    p.per = cfg->per;
    MlgAgentDims d{cfg->d_obs, cfg->A, cfg->N, cfg->H, c.d_in, cfg->obs_last_action, cfg->obs_agent_id};
    p.L = c.ff ? make_ff_layout(d) : make_agent_layout(d);
    p.ao = c.ff ? ff_offs(c.H, c.d_in, c.A) : agent_offs(c.H, c.d_in, c.A);
    p.mo = mix_offs(c.N, c.S, c.E, c.HE, p.layers);
    p.mp = mix_pack(c.N, c.S, c.E, c.HE, p.layers);
    p.n_agent = c.dx ? c.N * p.ao.total : p.ao.total;  // distinct: [agent 0 | ... | agent N - 1], then the mixer
    p.n_mixer = c.mixer == 2 ? p.mo.total : 0;
    WsLayout& w = p.w;
    const int64_t T = c.T, R = c.R, H = c.H, RM = c.RM;
    const bool one = p.layers == 1;  // mix_td1_kernel's rows: d1 = [b1 | vh], l1act = V's hidden activations
    const int L1 = one ? 2 * c.E : 2 * c.HE + 2 * c.E;
    int64_t o = 0;
    auto take = [&](int64_t n) { int64_t r = o; o += a4(n); return r; };
    // distinct networks: N blocks at DxView's strides. The [T][R][F] tensors below hold N instances of [T][B][F]
    // back to back, which is their size with R = B N
    w.p_on = take(c.dx ? (int64_t)c.N * p.L.gsp : p.L.total);
    w.p_tg = take(c.dx ? (int64_t)c.N * p.L.gsp : p.L.total);
    const int64_t G = c.ff ? 0 : 1;  // the feed-forward layout has no W_ih^T, gate, GI or gate-delta buffers
    w.wihT = take(G * 3 * H * H * (c.dx ? c.N : 1));
    w.mix_on = take(p.mp.total);
    w.mix_tg = take(p.mp.total);
    w.in = take(c.dx ? c.N * dx_in_stride(c) : T * R * c.d_in);
    w.x = take(G * T * R * H);
    // feed-forward: row block t + 1 holds relu(fc1) of step t (what agent_q_kernel reads); block 0 is never touched
    w.hs = take((T + 1) * R * H);
    w.hs_tg = take((T + 1) * R * H);
    w.gi_on = take(G * T * R * 3 * H);
    w.gi_tg = take(G * T * R * 3 * H);
    w.gr = take(G * T * R * H);
    w.gz = take(G * T * R * H);
    w.gn = take(G * T * R * H);
    w.ghn = take(G * T * R * H);
    w.mac = take(T * R * c.A);
    w.tmac = take(T * R * c.A);
    w.dq = take(T * R);
    w.d2 = take(T * R * c.A);
    w.dgi = take(G * T * R * 3 * H);
    w.dgh = take(G * T * R * 3 * H);
    w.da = take(T * R * H);
    w.srow = take(RM * c.S);
    w.l1act = take(RM * (one ? c.E : L1));
    w.d1 = take(RM * L1);
    w.da2 = take(RM * c.N * c.E);
    w.df2 = take(RM * c.E);
    w.dv2 = take(RM);
    w.hyp_stride = c.mixer == 2 ? (int)a4((int64_t)c.N * c.E + 2 * c.E + 1) : 0;  // mix_pre_tile rows (HypOut)
    w.hyp_on = take(RM * w.hyp_stride);
    w.hyp_tg = take(RM * w.hyp_stride);
    w.n_mix_tiles = (int)((RM + 15) / 16);
    w.part = take((int64_t)w.n_mix_tiles * 4);
    w.msum = take(4);
    w.rows = take(MLG_INLINE_ROWS);
    w.mlen = take(c.B);
    w.l16 = take((R + 15) / 16);
    w.flag = take(4);
    w.alive = take(c.dx ? c.N : 0);  // distinct networks: a word per slot (prep_kernel<true>)
    w.abits = take((T * R + 31) / 32);
    w.mbits = take((RM + 31) / 32);
    w.tdrow = take(p.per ? RM : 0);  // prioritized replay only: the rows' masked |td| (PerIo)
    w.nrm = 0;  // placed after the slab (size known once the jobs are built)
    w.slab = o;
    w.total = o;  // + slab size, filled by make_jobs
    return p;
}


// builds the job list; with ws == nullptr only sizes are computed (pointers are offsets from 0)
// distinct networks (rp != nullptr, filled here): the four agent jobs are those of one instance (T B rows, network 0's
// operands and gradient tensors) and repeat N times at the instances' strides (mlg::BRepeat); fc2's deltas are the
// mixer's d2 rows of the slot, N A floats apart
WJobs make_jobs(Plan& p, float* ws, float* grads, int64_t* slab_floats, int* n_tasks, int64_t* n_red,
                mlg::BRepeat* rp) {
    const LCfg& c = p.c;
    float* W = ws ? ws : nullptr;
    auto at = [&](int64_t off) { return W ? W + off : (float*)nullptr; };
    float* G = grads;
    auto gp = [&](int64_t off) { return G ? G + off : (float*)nullptr; };
    const int TR = c.T * (c.dx ? c.B : c.R), H = c.H, L1 = 2 * c.HE + 2 * c.E, RM = c.RM;
    const int Ra = c.dx ? c.B : c.R;  // agent rows per step of an instance
    WJobs J;
    J.n = 0;
    const AgentOffs& a = p.ao;
    J.j[J.n++] = mlg::bjob(at(p.w.da), H, at(p.w.in), c.d_in, gp(a.fc1w), gp(a.fc1b), H, c.d_in, TR);
    if (!c.ff) {
        J.j[J.n++] = mlg::bjob(at(p.w.dgi), 3 * H, at(p.w.x), H, gp(a.wih), gp(a.bih), 3 * H, H, TR);
        J.j[J.n++] = mlg::bjob(at(p.w.dgh), 3 * H, at(p.w.hs), H, gp(a.whh), gp(a.bhh), 3 * H, H, TR);
    }
    J.j[J.n++] = mlg::bjob(at(p.w.d2), c.dx ? (int64_t)c.N * c.A : c.A,
                           at(p.w.hs) ? at(p.w.hs) + (int64_t)Ra * H : nullptr, H, gp(a.fc2w), gp(a.fc2b), c.A, H, TR);
    const int n_agent_jobs = J.n;
    if (c.dx) {
        static_assert(mlg::MLG_BREP_JOBS >= 4, "the four agent jobs repeat");
        const int64_t TB = (int64_t)c.T * c.B;
        rp->rep = c.N;
        rp->nj = n_agent_jobs;
        rp->sg = a.total;
        rp->alive = reinterpret_cast<const unsigned*>(at(p.w.alive));
        const int64_t sd[4] = {TB * H, TB * 3 * H, TB * 3 * H, c.A};  // dA, dGI, dGH, d2 of the next slot
        const int64_t sx[4] = {dx_in_stride(c), TB * H, (TB + c.B) * H, (TB + c.B) * H};  // inputs, x, HS, HS[1..]
        for (int q = 0; q < 4; ++q) {
            rp->sd[q] = sd[q];
            rp->sx[q] = sx[q];
            J.j[q].va = J.j[q].va && sd[q] % 4 == 0;  // every repeat's rows readable as 16-byte vectors
            J.j[q].vb = J.j[q].vb && sx[q] % 4 == 0;
        }
        // a 16-byte load of fc2's delta columns past A would read the next slot's: element loads, guarded by M
        if (c.N > 1) J.j[3].va = 0;
    }
    if (c.mixer == 2 && p.layers == 1) {  // every delta against the state row; V.2 against V's hidden activations
        const MixOffs& m = p.mo;
        const int64_t G0 = p.n_agent;
        auto mg = [&](int64_t off) { return G ? G + G0 + off : (float*)nullptr; };
        const float* d1 = at(p.w.d1);
        auto off = [&](const float* base, int64_t k) { return base ? base + k : (const float*)nullptr; };
        const int NE = c.N * c.E;
        J.j[J.n++] = mlg::bjob(at(p.w.da2), NE, at(p.w.srow), c.S, mg(m.w1_0w), mg(m.w1_0b), NE, c.S, RM);
        J.j[J.n++] = mlg::bjob(at(p.w.df2), c.E, at(p.w.srow), c.S, mg(m.wf_0w), mg(m.wf_0b), c.E, c.S, RM);
        J.j[J.n++] = mlg::bjob(off(d1, 0), 2 * c.E, at(p.w.srow), c.S, mg(m.b1w), mg(m.b1b), c.E, c.S, RM);
        J.j[J.n++] = mlg::bjob(off(d1, c.E), 2 * c.E, at(p.w.srow), c.S, mg(m.v0w), mg(m.v0b), c.E, c.S, RM);
        J.j[J.n++] = mlg::bjob(at(p.w.dv2), 1, at(p.w.l1act), c.E, mg(m.v2w), mg(m.v2b), 1, c.E, RM);
    } else if (c.mixer == 2) {
        const MixOffs& m = p.mo;
        const int64_t G0 = p.n_agent;
        auto mg = [&](int64_t off) { return G ? G + G0 + off : (float*)nullptr; };
        const float* d1 = at(p.w.d1);
        const float* la = at(p.w.l1act);
        auto off = [&](const float* base, int64_t k) { return base ? base + k : (const float*)nullptr; };
        J.j[J.n++] = mlg::bjob(off(d1, 0), L1, at(p.w.srow), c.S, mg(m.w1_0w), mg(m.w1_0b), c.HE, c.S, RM);
        J.j[J.n++] = mlg::bjob(off(d1, c.HE), L1, at(p.w.srow), c.S, mg(m.wf_0w), mg(m.wf_0b), c.HE, c.S, RM);
        J.j[J.n++] = mlg::bjob(off(d1, 2 * c.HE), L1, at(p.w.srow), c.S, mg(m.b1w), mg(m.b1b), c.E, c.S, RM);
        J.j[J.n++] = mlg::bjob(off(d1, 2 * c.HE + c.E), L1, at(p.w.srow), c.S, mg(m.v0w), mg(m.v0b), c.E, c.S, RM);
        J.j[J.n++] = mlg::bjob(at(p.w.da2), (int64_t)c.N * c.E, off(la, 0), L1, mg(m.w1_2w), mg(m.w1_2b), c.N * c.E, c.HE, RM);
        J.j[J.n++] = mlg::bjob(at(p.w.df2), c.E, off(la, c.HE), L1, mg(m.wf_2w), mg(m.wf_2b), c.E, c.HE, RM);
        J.j[J.n++] = mlg::bjob(at(p.w.dv2), 1, off(la, 2 * c.HE + c.E), L1, mg(m.v2w), mg(m.v2b), 1, c.E, RM);
    }
    // every job loads live rows only (Skip): the agent's t-major rows by their 16-row tile's steps, the mixer's
    // (b, t) rows by the episode's live transitions. Chunks stay contiguous: each sum keeps its order.
    for (int q = 0; q < J.n; ++q) {
        const float* bits = at(q < n_agent_jobs ? p.w.abits : p.w.mbits);
        J.j[q] = mlg::bjob_row_bits(J.j[q], reinterpret_cast<const uint32_t*>(bits));
    }
    int64_t slab_part;
    *slab_floats = mlg::layout_bjobs(J, n_tasks, n_red, &slab_part, c.dx ? rp : nullptr);  // slab + per-block norm partials
    p.w.nrm = p.w.slab + slab_part;
    return J;
}

// ---- dispatch: every shape-dependent choice of a call, decided once on the host. run_train launches what this
// says and mlg_qlearner_describe prints it, so the query cannot drift from the launches.
enum MixKernel {
    MIX_IQL,         // iql_td_kernel
    MIX_VDN_FAST,    // mix_td_kernel<64, 32, true>, mixer 1
    MIX_VDN,         // mix_td_kernel<64, 32>, mixer 1
    MIX_QMIX_SPLIT,  // rec4_mixpre_kernel<H> + mix_td2_kernel<64, 32>
    MIX_QMIX_FAST1,  // mix_td_kernel<64, 32, true>, mixer 2: needs threads % 128 != 0, which no H gives
    MIX_QMIX_DFLT,   // mix_td_kernel<64, 32>, mixer 2
    MIX_QMIX1,       // mix_td1_kernel<E>
    MIX_QMIX_WIDTHS  // mix_td_kernel<HE, E>, the other widths
};
struct Dispatch {
    bool dflt_mix, fast_mix, split_mix, fused;
    int threads;  // workgroup size of the per-H agent kernels
    int q_tiles;  // 16-action tiles: agent_q_kernel runs 64 q_tiles threads
    int per;      // mixer tiles per workgroup of rec4_mixpre_kernel (split_mix)
    MixKernel mix;
    static constexpr bool fused_for(int H) { return H == 64; }  // 4 waves, as the wgrad workgroups
};

// MLG_MIX_GENERIC is read per call, so a test can set it. Nonzero (mlg_last_error) where no mixer kernel exists.
int make_dispatch(const Plan& p, Dispatch* out) {
    const LCfg& c = p.c;
    Dispatch d;
    // split mixer (default for the FAST shapes): the hypernetwork forward rides in the recurrence launch
    // (rec4_mixpre_kernel), mix_td2_kernel does the rest. VDN runs the one-kernel mix_td; MLG_MIX_GENERIC=1
    // forces its generic form (the path of the other shapes)
    d.dflt_mix = c.mixer == 1 || (c.mixer == 2 && p.layers == 2 && c.E == 32 && c.HE == 64);
    d.fast_mix = d.dflt_mix && p.mp.Sp <= 64 && c.N <= MIXPF_N && c.A <= MIXPF_A && !getenv("MLG_MIX_GENERIC");
    // feed-forward: no recurrence launch for the hypernet forward to ride in, so QMIX runs its one-kernel generic form
    if (c.ff && c.mixer == 2) d.fast_mix = false;
    // distinct networks: the split form's hypernet tiles ride in the shared agent's recurrence launch and the fused
    // backward carries the shared agent's job views; neither is carried over (QMIX runs its one-kernel generic form,
    // the weight gradients one launch after agent_dx). The mixer kernels themselves are the shared agent's.
    if (c.dx && c.mixer == 2) d.fast_mix = false;
    d.threads = (c.H / 16) * 64;
    d.split_mix = c.mixer == 2 && d.fast_mix && d.threads % 128 == 0;
    d.per = d.threads / 128;
    d.q_tiles = c.Ap / 16;
    d.fused = !c.ff && !c.dx && Dispatch::fused_for(c.H);
    if (c.mixer == 0) {
        d.mix = MIX_IQL;
    } else if (d.split_mix) {
        d.mix = MIX_QMIX_SPLIT;
    } else if (d.fast_mix) {
        d.mix = c.mixer == 1 ? MIX_VDN_FAST : MIX_QMIX_FAST1;
    } else if (c.mixer == 2 && p.layers == 1) {  // widths checked by check_cfg
        d.mix = MIX_QMIX1;
    } else if (d.dflt_mix) {
        d.mix = c.mixer == 1 ? MIX_VDN : MIX_QMIX_DFLT;
    } else {  // the other widths: the generic one-kernel form only
        const bool he_ok = c.HE == 32 || c.HE == 64 || c.HE == 128, e_ok = c.E == 16 || c.E == 32 || c.E == 64;
        if (!he_ok || !e_ok) return mlg::fail("learner: no mixer kernel for hypernet_embed=%d mixing_embed_dim=%d", c.HE, c.E);
        d.mix = MIX_QMIX_WIDTHS;
    }
    *out = d;
    return 0;
}

// "<agent part> + <mixer part>" of a dispatch (mlg_qlearner_describe; the names are listed in maleague.h)
void dispatch_name(const LCfg& c, const Dispatch& d, int per, char* name, size_t cap) {
    char mix[40];
    switch (d.mix) {
        case MIX_IQL: snprintf(mix, sizeof mix, "iql"); break;
        case MIX_VDN_FAST: snprintf(mix, sizeof mix, "vdn-fast"); break;
        case MIX_VDN: snprintf(mix, sizeof mix, "vdn"); break;
        case MIX_QMIX_SPLIT: snprintf(mix, sizeof mix, "qmix-split"); break;
        case MIX_QMIX_FAST1: snprintf(mix, sizeof mix, "qmix-fast1"); break;
        case MIX_QMIX_DFLT: snprintf(mix, sizeof mix, "qmix-generic"); break;
        case MIX_QMIX1: snprintf(mix, sizeof mix, "qmix1-e%d", c.E); break;
        case MIX_QMIX_WIDTHS: snprintf(mix, sizeof mix, "qmix-he%d-e%d", c.HE, c.E); break;
    }
    if (per) strcat(mix, " + per");  // the PER forms of the TD kernel and per_reduce_kernel
    if (c.ff) snprintf(name, cap, "ff-h%d/q%d + %s", c.H, d.q_tiles, mix);
    else if (c.dx) snprintf(name, cap, "dx-h%d/bwd-split/q%d + %s", c.H, d.q_tiles, mix);
    else snprintf(name, cap, "h%d/%s/q%d + %s", c.H, d.fused ? "bwd-fused" : "bwd-split", d.q_tiles, mix);
}

// the one reduce over the job table, then clip + RMSprop + statistics (both agents end a call the same way)
int run_finish(const Plan& p, const MlgLearnerCfg* cfg, const MlgLearnerBufs* bufs, hipStream_t s, const WJobs& J,
               int64_t n_red, unsigned* flag, const Skip& sk, int ntiles, const mlg::BRepeat* rp = nullptr) {
    const LCfg& c = p.c;
    float* ws = bufs->workspace;
    const int n_red_blocks = (int)((n_red + 255) / 256);
    if (rp)
        hipLaunchKernelGGL(mlg::wgrad_block_reduce_rep_kernel<16>, dim3((unsigned)n_red_blocks), dim3(256), 0, s, J, *rp,
                           ws + p.w.slab, ws + p.w.nrm);
    else
        hipLaunchKernelGGL(mlg::wgrad_block_reduce_kernel<16>, dim3((unsigned)n_red_blocks), dim3(256), 0, s, J,
                           ws + p.w.slab, ws + p.w.nrm);
    const int64_t n_par = p.n_agent + p.n_mixer;
    hipLaunchKernelGGL(finish_kernel, dim3((unsigned)((n_par + 1023) / 1024)), dim3(1024), 0, s, ws + p.w.part,
                       p.w.n_mix_tiles, ws + p.w.msum + (c.mixer == 0 ? 2 : 0), bufs->params, bufs->grads, bufs->square_avg, n_par, cfg->lr,
                       cfg->optim_alpha, cfg->optim_eps, cfg->grad_norm_clip, c.N, bufs->stats, ws + p.w.nrm,
                       n_red_blocks, bufs->target_sync, bufs->trained_steps, sk, flag, ntiles, c.full, c.dx ? c.N : 1);
    return mlg::check_launch("qlearner_train");
}

template <int H>
int run_train(Plan& p, const MlgLearnerCfg* cfg, const MlgLearnerBufs* bufs, hipStream_t s) {
    const LCfg& c = p.c;
    Dispatch dsp;
    if (make_dispatch(p, &dsp)) return 1;
    float* ws = bufs->workspace;
    MlgBatch bt = bufs->batch;
    int32_t* rows_ws = reinterpret_cast<int32_t*>(ws + p.w.rows);
    if (bufs->host_rows) bt.rows = rows_ws;  // filled by prep_kernel's block 0 from its argument
    const float* params = bufs->params;
    const float* tparams = bufs->target_params;
    // ---- fused prologue: pack online / target agent + mixer, W_ih^T, zero d2 / dq, mask sum ----
    auto agent_ptrs = [&](const float* flat) {
        return MlgAgentParams{flat + p.ao.fc1w, flat + p.ao.fc1b, flat + p.ao.wih, flat + p.ao.bih,
                              flat + p.ao.whh, flat + p.ao.bhh, flat + p.ao.fc2w, flat + p.ao.fc2b};
    };
    PrepJob pj;
    pj.L = p.L;
    pj.ap_on = agent_ptrs(params);
    pj.ap_tg = agent_ptrs(tparams);
    pj.p_on = ws + p.w.p_on;
    pj.p_tg = ws + p.w.p_tg;
    pj.wih = params + p.ao.wih;
    pj.wihT = ws + p.w.wihT;
    pj.rows3 = c.ff ? 0 : 3 * c.H;  // feed-forward: no W_ih^T
    pj.cols = c.H;
    pj.ff = c.ff;
    pj.mp = p.mp;
    pj.mo = p.mo;
    pj.mix_src_on = params + p.n_agent;
    pj.mix_src_tg = tparams + p.n_agent;
    pj.mix_on = ws + p.w.mix_on;
    pj.mix_tg = ws + p.w.mix_tg;
    pj.N = c.dx ? 1 : c.N;  // distinct networks: the Skip tables of one instance (R = B rows, one agent each)
    pj.nag = c.dx ? c.N : 1;
    pj.nslots = c.N;
    pj.A = c.A;
    pj.ao_total = p.ao.total;
    pj.alive = reinterpret_cast<unsigned*>(ws + p.w.alive);
    pj.S = c.S;
    pj.E = c.E;
    pj.HE = c.HE;
    pj.mixer = c.mixer;
    const int threads = dsp.threads;
    const bool split_mix = dsp.split_mix;
    pj.d2 = ws + p.w.d2;  // d2 is sparse: zero it (and dq) every call
    pj.dq = ws + p.w.dq;
    pj.n_d2 = (int64_t)c.T * c.R * c.A;
    pj.n_dq = (int64_t)c.T * c.R;
    pj.bt = bt;
    pj.B = c.B;
    pj.T = c.T;
    pj.msum = ws + p.w.msum;
    pj.mlen = ws + p.w.mlen;
    pj.l16 = ws + p.w.l16;
    pj.flag = reinterpret_cast<unsigned*>(ws + p.w.flag);
    pj.abits = reinterpret_cast<uint32_t*>(ws + p.w.abits);
    pj.mbits = reinterpret_cast<uint32_t*>(ws + p.w.mbits);
    pj.cmp_on = params;
    pj.cmp_tg = tparams;
    pj.n_cmp = p.n_agent + p.n_mixer;
    pj.cmp_vec = ((uintptr_t)params % 16 == 0) && ((uintptr_t)tparams % 16 == 0);
    pj.R = c.dx ? c.B : c.R;
    pj.full = c.full;
    const Skip sk{pj.mlen, pj.l16, pj.flag};
    pj.n_rows_in = 0;
    pj.rows_dst = rows_ws;
    if (bufs->host_rows) {
        pj.n_rows_in = c.B;
        for (int b = 0; b < c.B; ++b) pj.rows_in[b] = bufs->host_rows[b];
    }
    if (c.dx) {  // block 0 the tables, blocks 1 .. N the slots' liveness, the others the N networks' packs and the rest
        const int64_t work = c.N * (2 * (int64_t)p.L.gsp + (int64_t)pj.rows3 * c.H) + (c.mixer == 2 ? 2 * p.mp.total : 0) +
                             pj.n_d2 + pj.n_dq + (pj.n_cmp + 3) / 4;
        const int blocks = 1 + c.N + (int)std::min<int64_t>((work + 1023) / 1024, 512);
        hipLaunchKernelGGL(prep_kernel<true>, dim3(blocks), dim3(1024), 0, s, pj);
    } else {
        const int64_t work = 2 * p.L.total + (int64_t)pj.rows3 * c.H + (c.mixer == 2 ? 2 * p.mp.total : 0) + pj.n_d2 +
                             pj.n_dq + (pj.n_cmp + 3) / 4;
        const int blocks = 1 + (int)std::min<int64_t>((work + 1023) / 1024, 512);
        hipLaunchKernelGGL(prep_kernel<false>, dim3(blocks), dim3(1024), 0, s, pj);
    }
    MixPtrs Mon{}, Mtg{};
    if (c.mixer == 2) {
        const int64_t g0 = p.n_agent;
        auto ptrs = [&](const float* flat, const float* pk) {
            MixPtrs m;
            m.m1 = pk + p.mp.m1;
            m.mb1 = pk + p.mp.mb1;
            m.a2 = flat + g0 + p.mo.w1_2w;
            m.ba2 = flat + g0 + p.mo.w1_2b;
            m.a2T = pk + p.mp.a2T;
            m.f2 = flat + g0 + p.mo.wf_2w;
            m.bf2 = flat + g0 + p.mo.wf_2b;
            m.f2T = pk + p.mp.f2T;
            m.v2p = pk + p.mp.v2p;
            m.bv2p = pk + p.mp.bv2p;
            return m;
        };
        Mon = ptrs(params, ws + p.w.mix_on);
        Mtg = ptrs(tparams, ws + p.w.mix_tg);
    }
    const int Ra = c.dx ? c.B : c.R;  // agent rows of an instance (distinct networks: N instances, a grid coordinate)
    const int ntiles = (Ra + 15) / 16;
    HypOut hy{ws + p.w.hyp_on, ws + p.w.hyp_tg, ws + p.w.l1act, ws + p.w.srow, p.w.hyp_stride};
    if (c.dx) {
        hipLaunchKernelGGL((agent_in_kernel<H, true>), dim3(ntiles, c.T, 2 * c.N), dim3(threads), 0, s, c, bt, p.L,
                           ws + p.w.p_on, ws + p.w.p_tg, ws + p.w.in, ws + p.w.x, ws + p.w.gi_on, ws + p.w.gi_tg, sk);
        hipLaunchKernelGGL((agent_rec4_kernel<H, true>), dim3(2 * ((Ra + 3) / 4), c.N), dim3(threads), 0, s, c, p.L,
                           ws + p.w.p_on, ws + p.w.p_tg, ws + p.w.gi_on, ws + p.w.gi_tg, ws + p.w.hs, ws + p.w.hs_tg,
                           ws + p.w.gr, ws + p.w.gz, ws + p.w.gn, ws + p.w.ghn, sk);
        hipLaunchKernelGGL((agent_q_kernel<H, true>), dim3(ntiles, c.T, 2 * c.N), dim3(64 * dsp.q_tiles), 0, s, c, p.L,
                           ws + p.w.p_on, ws + p.w.p_tg, ws + p.w.hs, ws + p.w.hs_tg, ws + p.w.mac, ws + p.w.tmac, sk);
    } else if (c.ff)
        hipLaunchKernelGGL((ff_hidden_kernel<H>), dim3(ntiles, c.T, 2), dim3(threads), 0, s, c, bt, p.L, ws + p.w.p_on,
                           ws + p.w.p_tg, ws + p.w.in, ws + p.w.hs, ws + p.w.hs_tg, sk);
    else
        hipLaunchKernelGGL((agent_in_kernel<H>), dim3(ntiles, c.T, 2), dim3(threads), 0, s, c, bt, p.L, ws + p.w.p_on,
                           ws + p.w.p_tg, ws + p.w.in, ws + p.w.x, ws + p.w.gi_on, ws + p.w.gi_tg, sk);
    if (c.ff || c.dx) {
        // feed-forward: no recurrence, the hidden rows are complete; distinct networks: launched above
    } else if (split_mix) {
        const int nrec = 2 * ((c.R + 3) / 4), per = dsp.per;
        hipLaunchKernelGGL((rec4_mixpre_kernel<H>), dim3(nrec + (p.w.n_mix_tiles + per - 1) / per), dim3(threads), 0, s,
                           c, p.L, ws + p.w.p_on, ws + p.w.p_tg, ws + p.w.gi_on, ws + p.w.gi_tg, ws + p.w.hs,
                           ws + p.w.hs_tg, ws + p.w.gr, ws + p.w.gz, ws + p.w.gn, ws + p.w.ghn, sk, bt, Mon,
                           Mtg, p.mp, hy);
    } else
        hipLaunchKernelGGL((agent_rec4_kernel<H>), dim3(2 * ((c.R + 3) / 4)), dim3(threads), 0, s, c, p.L,
                           ws + p.w.p_on, ws + p.w.p_tg, ws + p.w.gi_on, ws + p.w.gi_tg, ws + p.w.hs, ws + p.w.hs_tg,
                           ws + p.w.gr, ws + p.w.gz, ws + p.w.gn, ws + p.w.ghn, sk);
    if (!c.dx)
        hipLaunchKernelGGL((agent_q_kernel<H>), dim3(ntiles, c.T, 2), dim3(64 * dsp.q_tiles), 0, s, c, p.L, ws + p.w.p_on,
                           ws + p.w.p_tg, ws + p.w.hs, ws + p.w.hs_tg, ws + p.w.mac, ws + p.w.tmac, sk);
    MixOut mo{ws + p.w.srow, ws + p.w.l1act, ws + p.w.d1, ws + p.w.da2, ws + p.w.df2, ws + p.w.dv2,
              ws + p.w.dq, ws + p.w.d2, ws + p.w.part};
    // prioritized replay: the <.., true> form of the same kernel, then the per-episode reduce. <.., false> is the
    // instantiation the defaulted template arguments name: an unweighted call launches what it always has.
    const bool per = p.per != 0;
    const PerIo pw{per ? bufs->is_weight : nullptr, per ? ws + p.w.tdrow : nullptr};
#define MLG_MIX_LAUNCH_K(K)                                                                                     \
    hipLaunchKernelGGL((K), dim3(p.w.n_mix_tiles), dim3(128), 0, s, c, bt, Mon, Mtg, p.mp, ws + p.w.mac, ws + p.w.tmac, \
                       ws + p.w.msum, mo, sk, pw)
#define MLG_MIX_LAUNCH(K, ...)                                     \
    do {                                                           \
        if (per) MLG_MIX_LAUNCH_K((K<__VA_ARGS__, true>));         \
        else MLG_MIX_LAUNCH_K((K<__VA_ARGS__, false>));            \
    } while (0)
    switch (dsp.mix) {
        case MIX_IQL:
            if (per)
                hipLaunchKernelGGL(iql_td_kernel<true>, dim3(p.w.n_mix_tiles), dim3(64), 0, s, c, bt, ws + p.w.mac,
                                   ws + p.w.tmac, ws + p.w.msum, mo, sk, pw);
            else
                hipLaunchKernelGGL(iql_td_kernel<false>, dim3(p.w.n_mix_tiles), dim3(64), 0, s, c, bt, ws + p.w.mac,
                                   ws + p.w.tmac, ws + p.w.msum, mo, sk, pw);
            break;
        case MIX_QMIX_SPLIT:
            if (per)
                hipLaunchKernelGGL((mix_td2_kernel<64, 32, true>), dim3(p.w.n_mix_tiles), dim3(128), 0, s, c, bt, Mon,
                                   ws + p.w.mac, ws + p.w.tmac, ws + p.w.msum, hy, mo, sk, pw);
            else
                hipLaunchKernelGGL((mix_td2_kernel<64, 32, false>), dim3(p.w.n_mix_tiles), dim3(128), 0, s, c, bt, Mon,
                                   ws + p.w.mac, ws + p.w.tmac, ws + p.w.msum, hy, mo, sk, pw);
            break;
        case MIX_VDN_FAST:
        case MIX_QMIX_FAST1: MLG_MIX_LAUNCH(mix_td_kernel, 64, 32, true); break;
        case MIX_QMIX1:
            if (c.E == 16) MLG_MIX_LAUNCH(mix_td1_kernel, 16);
            else if (c.E == 32) MLG_MIX_LAUNCH(mix_td1_kernel, 32);
            else MLG_MIX_LAUNCH(mix_td1_kernel, 64);
            break;
        case MIX_VDN:
        case MIX_QMIX_DFLT: MLG_MIX_LAUNCH(mix_td_kernel, 64, 32, false); break;
        case MIX_QMIX_WIDTHS:
            switch (c.HE * 1000 + c.E) {
                case 32016: MLG_MIX_LAUNCH(mix_td_kernel, 32, 16, false); break;
                case 32032: MLG_MIX_LAUNCH(mix_td_kernel, 32, 32, false); break;
                case 32064: MLG_MIX_LAUNCH(mix_td_kernel, 32, 64, false); break;
                case 64016: MLG_MIX_LAUNCH(mix_td_kernel, 64, 16, false); break;
                case 64064: MLG_MIX_LAUNCH(mix_td_kernel, 64, 64, false); break;
                case 128016: MLG_MIX_LAUNCH(mix_td_kernel, 128, 16, false); break;
                case 128032: MLG_MIX_LAUNCH(mix_td_kernel, 128, 32, false); break;
                case 128064: MLG_MIX_LAUNCH(mix_td_kernel, 128, 64, false); break;
                default: return mlg::fail("learner: no mixer kernel for hypernet_embed=%d mixing_embed_dim=%d", c.HE, c.E);
            }
            break;
    }
#undef MLG_MIX_LAUNCH
#undef MLG_MIX_LAUNCH_K
    if (per)
        hipLaunchKernelGGL(per_reduce_kernel, dim3(c.B), dim3(64), 0, s, c, bt, ws + p.w.tdrow, sk,
                           c.mixer == 0 ? (float)c.N : 1.f, bufs->td_abs);
    // weight gradients: fc2 and the mixer's jobs (final after the mixer kernel, table view JA) run as extra
    // workgroups of the reverse-recurrence launch (H = 64, bwd4_wgrad_kernel); fc1 / W_ih / W_hh (view JB) after
    // agent_dx; one reduce over the whole table
    int64_t slab_floats, n_red;
    int n_tasks;
    mlg::BRepeat rp{};
    WJobs J = make_jobs(p, ws, bufs->grads, &slab_floats, &n_tasks, &n_red, &rp);
    if (c.dx) {
        // distinct networks: the N reverse recurrences and dX passes by grid coordinate, then every job in one launch
        // (the agent jobs repeat per network) and the one reduce, which zeroes a dead slot's network
        hipLaunchKernelGGL((agent_bwd4_kernel<H, true>), dim3((Ra + 3) / 4, c.N), dim3(threads), 0, s, c, bt, p.L,
                           ws + p.w.p_on, ws + p.w.hs, ws + p.w.gr, ws + p.w.gz, ws + p.w.gn, ws + p.w.ghn, ws + p.w.dq,
                           ws + p.w.dgi, ws + p.w.dgh, sk);
        hipLaunchKernelGGL((agent_dx_kernel<H, true>), dim3(ntiles, c.T, c.N), dim3(threads), 0, s, c, ws + p.w.wihT,
                           ws + p.w.x, ws + p.w.dgi, ws + p.w.da, sk);
        hipLaunchKernelGGL(mlg::wgrad_block_rep_kernel<16>, dim3((unsigned)((n_tasks + 3) / 4)), dim3(256), 0, s, J, rp,
                           ws + p.w.slab);
        return run_finish(p, cfg, bufs, s, J, n_red, pj.flag, sk, ntiles, &rp);
    }
    if (c.ff) {
        // feed-forward: the fc1 delta rows, then every job in one launch and the one reduce
        hipLaunchKernelGGL((ff_bwd_kernel<H>), dim3(ntiles, c.T), dim3(threads), 0, s, c, p.L, ws + p.w.p_on, ws + p.w.hs,
                           ws + p.w.d2, ws + p.w.da, sk);
        hipLaunchKernelGGL(mlg::wgrad_block_kernel<16>, dim3((unsigned)((n_tasks + 3) / 4)), dim3(256), 0, s, J,
                           ws + p.w.slab);
        return run_finish(p, cfg, bufs, s, J, n_red, pj.flag, sk, ntiles);
    }
    int ta, tb;
    int64_t ra, rb;
    const WJobs JA = mlg::bjob_view(J, 3, J.n, &ta, &ra), JB = mlg::bjob_view(J, 0, 3, &tb, &rb);
    constexpr bool fused = Dispatch::fused_for(H);  // == dsp.fused
    if constexpr (fused) {
        const int nbwd = (c.R + 3) / 4;
        hipLaunchKernelGGL((bwd4_wgrad_kernel<H>), dim3((unsigned)(nbwd + (ta + 3) / 4)), dim3(256), 0, s, c, bt, p.L,
                           ws + p.w.p_on, ws + p.w.hs, ws + p.w.gr, ws + p.w.gz, ws + p.w.gn, ws + p.w.ghn, ws + p.w.dq,
                           ws + p.w.dgi, ws + p.w.dgh, sk, JA, ws + p.w.slab, nbwd);
    } else {
        hipLaunchKernelGGL((agent_bwd4_kernel<H>), dim3((c.R + 3) / 4), dim3(threads), 0, s, c, bt, p.L, ws + p.w.p_on,
                           ws + p.w.hs, ws + p.w.gr, ws + p.w.gz, ws + p.w.gn, ws + p.w.ghn, ws + p.w.dq, ws + p.w.dgi,
                           ws + p.w.dgh, sk);
    }
    hipLaunchKernelGGL((agent_dx_kernel<H>), dim3(ntiles, c.T), dim3(threads), 0, s, c, ws + p.w.wihT, ws + p.w.x,
                       ws + p.w.dgi, ws + p.w.da, sk);
    if (fused)
        hipLaunchKernelGGL(mlg::wgrad_block_kernel<16>, dim3((unsigned)((tb + 3) / 4)), dim3(256), 0, s, JB,
                           ws + p.w.slab);
    else
        hipLaunchKernelGGL(mlg::wgrad_block_kernel<16>, dim3((unsigned)((n_tasks + 3) / 4)), dim3(256), 0, s, J,
                           ws + p.w.slab);
    return run_finish(p, cfg, bufs, s, J, n_red, pj.flag, sk, ntiles);
}

}  // namespace

extern "C" int mlg_debug_set_learner_stamps(void* ptr) {
#ifdef MLG_STAMPS
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(g_mlg_lstamps), &ptr, sizeof(ptr));
    if (e != hipSuccess) return mlg::fail("set learner stamps: %s", hipGetErrorString(e));
    return 0;
#else
    (void)ptr;
    return mlg::fail("not a stamps build (-DMLG_STAMPS)");
#endif
}

extern "C" int64_t mlg_qlearner_param_counts(const MlgLearnerCfg* c, int64_t* n_agent, int64_t* n_mixer) {
    if (check_cfg(c)) return -1;
    Plan p = make_plan(c, c->T);
    if (n_agent) *n_agent = p.n_agent;
    if (n_mixer) *n_mixer = p.n_mixer;
    return p.n_agent + p.n_mixer;
}

extern "C" int mlg_qlearner_inline_rows(void) { return MLG_INLINE_ROWS; }

extern "C" int64_t mlg_qlearner_workspace_floats(const MlgLearnerCfg* c) {
    if (check_cfg(c)) return -1;
    Plan p = make_plan(c, c->T);
    int64_t slab, n_red;
    int tasks;
    mlg::BRepeat rp{};
    make_jobs(p, nullptr, nullptr, &slab, &tasks, &n_red, &rp);
    return p.w.total + slab;
}

extern "C" int mlg_qlearner_describe(const MlgLearnerCfg* c, char* name, int32_t name_cap) {
    if (check_cfg(c)) return 1;
    MLG_REQUIRE(name && name_cap > 0, "qlearner_describe: null output");
    Plan p = make_plan(c, c->T);
    Dispatch d;
    if (make_dispatch(p, &d)) return 1;
    char full[64];
    dispatch_name(p.c, d, p.per, full, sizeof full);
    MLG_REQUIRE((size_t)name_cap > strlen(full), "qlearner_describe: name buffer of %d bytes too small", name_cap);
    strcpy(name, full);
    return 0;
}

extern "C" int mlg_qlearner_train(const MlgLearnerCfg* c, const MlgLearnerBufs* b, void* stream) {
    if (check_cfg(c)) return 1;
    MLG_REQUIRE(b && b->params && b->grads && b->square_avg && b->target_params && b->workspace && b->stats,
                "qlearner_train: null buffer");
    const MlgBatch& bt = b->batch;
    MLG_REQUIRE(bt.state && bt.obs && bt.actions && bt.avail && bt.reward && bt.terminated && bt.actions_onehot && bt.filled,
                "qlearner_train: batch has null tensors");
    MLG_REQUIRE(bt.B == c->B && bt.T1 >= c->T, "qlearner_train: batch B=%d T1=%d vs cfg B=%d T=%d", bt.B, bt.T1, c->B, c->T);
    MLG_REQUIRE(!b->host_rows || c->B <= MLG_INLINE_ROWS, "qlearner_train: host_rows needs B <= %d (got %d)",
                MLG_INLINE_ROWS, c->B);
    MLG_REQUIRE(!c->per || (b->is_weight && b->td_abs), "qlearner_train: per=1 needs is_weight and td_abs");
    Plan p = make_plan(c, bt.T1);
    hipStream_t s = (hipStream_t)stream;
    if (c->H == 64) return run_train<64>(p, c, b, s);
    if (c->H == 32) return run_train<32>(p, c, b, s);
    return run_train<128>(p, c, b, s);
}
