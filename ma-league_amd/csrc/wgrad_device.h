// wgrad_device.h -- weight gradients as job lists, shared by the QMIX and REFIL learners:
// dW[M][K] = sum_rows delta[row][m] x[row][k], db[m] = sum_rows delta[row][m]: one wave per (job, 64 x 64 output
// block, row chunk of up to 1024 rows), MFMA with the row index as K; per 32-row step every lane loads 4 delta and
// 4 x values of 8 rows and issues 16 MFMA groups. The 4 waves of a workgroup (4 chunks of one block) add their
// partials in LDS; the partials [block][chunk group][64 * 64 + 64] are summed over groups in a fixed order
// (deterministic). The reduce pass also emits per-block sums of squares for clip_grad_norm_, which the learners'
// finish kernels turn into the clipped RMSprop step (clip_rmsprop_step).
#pragma once
#include "mlg_device.h"
#include "mlg_host.h"

// helpers of the stand-alone backward row passes (agent_grad.hip, refil_grad.hip)
__device__ __forceinline__ void st4(float* p, floatx4 v) { *reinterpret_cast<floatx4*>(p) = v; }
// Column m of four consecutive weight rows k0 .. k0 + 3: the A operand of a transposed product (out = W^T . delta),
// K slots in the order of the D layout (feature 16c + 4g + r at step (c, r)).
__device__ __forceinline__ floatx4 ld_col4(const float* w, int64_t k0, int ld, int m) {
    const float* p = w + k0 * ld + m;
    return floatx4{p[0], p[ld], p[2 * (int64_t)ld], p[3 * (int64_t)ld]};
}

namespace mlg {

__device__ __forceinline__ float block_sum_1024(float v, float* red) {
    // deterministic sum over blockDim.x (a multiple of 64, <= 1024) threads, result in every thread: a butterfly
    // within each wave (lane 0's fixed association), then the waves' partials in wave order -- two barriers instead
    // of one per tree level
    const int tid = threadIdx.x, nw = (int)(blockDim.x >> 6);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float r = 0.f;
    for (int i = 0; i < nw; ++i) r += red[i];
    __syncthreads();  // red reusable by the caller
    return r;
}

constexpr int BCH = 1024;        // max rows per chunk
constexpr int BSLAB = 64 * 64 + 64;
constexpr int MLG_WRED_DEPTH = 64;  // slab partials in flight per thread of the reduce pass

struct BJob {
    const float* delta;
    const float* x;
    float* dw;
    float* db;
    int64_t ldd, ldx;
    int M, K, rows, mb, nb, chunks, ch_rows;
    int va, vb;  // delta / x rows readable as 16-byte vectors (ld % 4 == 0, 16-byte aligned base)
    int task0;
    int64_t slab0;
    // rows with an exactly zero delta skipped (REFIL learner: items past each sampled episode's live steps, whose
    // deltas the backward kernels write as zeros): 0 off; 1 item-major rows, item = (row / rpi) % I, (b, t) = (item / T,
    // item % T); 2 t-major rows, t = row / R, b = ((row % R) / NA) % B. Row r is live iff t < mlen[b]. Groups of 8
    // consecutive rows share one (b, t) (rpi, NA and R multiples of 8).
    // 3 (QMIX learner): liveness per row from a bitmap (`mlen` holds uint32 words, bit row % 32 of word row / 32; a
    // 32-row step's liveness is one word, no division and no table walk in the kernel). Chunks stay contiguous, so
    // every sum keeps its order. Dead rows are never loaded: neither their deltas nor their x rows need to exist.
    int skip, rpi, I, T, R, NA, B;
    const float* mlen;
};
template <int MJ>
struct BJobsT {
    BJob j[MJ];
    int n;
};

// Repeated jobs (the QMIX learner with distinct per-agent networks): jobs [0, nj) of a table run `rep` times, repeat a
// on operands shifted by a sd[q] (delta) and a sx[q] (x) floats, into dw / db shifted by a sg; the other jobs run once.
// A repeat is a job of its own in every respect (tasks, slab partials, chunk order: each sum is the one the job would
// give alone on the shifted operands), so a table of 16 jobs covers any number of networks. alive (nullptr = all): a
// repeat with alive[a] == 0 stores exact zeros for dw / db and adds nothing to the norm (reduce pass). A separate
// kernel argument of the *_rep kernels: tables without repeats travel and run as before.
constexpr int MLG_BREP_JOBS = 4;
struct BRepeat {
    int rep, nj;
    int64_t sd[MLG_BREP_JOBS], sx[MLG_BREP_JOBS], sg;
    const unsigned* alive;
};

inline BJob bjob(const float* delta, int64_t ldd, const float* x, int64_t ldx, float* dw, float* db, int M, int K,
                 int rows) {
    BJob j;
    j.delta = delta;
    j.x = x;
    j.dw = dw;
    j.db = db;
    j.ldd = ldd;
    j.ldx = ldx;
    j.M = M;
    j.K = K;
    j.rows = rows;
    j.mb = (M + 63) / 64;
    j.nb = (K + 63) / 64;
    // chunk length: up to BCH rows, fewer when the job is small so that it still spreads over >= ~256 waves
    constexpr int target = 256;  // waves per job
    int ch = rows / (target / (j.mb * j.nb) + 1);
    ch = ch < 64 ? 64 : (ch > BCH ? BCH : ch);
    j.ch_rows = (ch + 31) & ~31;  // whole 32-row MFMA steps
    j.va = (ldd % 4 == 0) && ((uintptr_t)delta % 16 == 0);
    j.vb = (ldx % 4 == 0) && ((uintptr_t)x % 16 == 0);
    j.chunks = (rows + j.ch_rows - 1) / j.ch_rows;
    j.task0 = 0;
    j.slab0 = 0;
    j.skip = 0;
    j.rpi = j.I = j.T = j.R = j.NA = j.B = 1;
    j.mlen = nullptr;
    return j;
}

// skip rows with zero deltas (see BJob::skip); item-major rows of rpi rows per item over I items of T steps
inline BJob bjob_items(BJob j, const float* mlen, int rpi, int I, int T) {
    j.skip = 1;
    j.mlen = mlen;
    j.rpi = rpi;
    j.I = I;
    j.T = T;
    return j;
}
// t-major rows: R rows per step, row r of a step belongs to episode (r / NA) % B
// per-row liveness (BJob::skip 3): bit row % 32 of bits[row / 32], (rows + 31) / 32 words
inline BJob bjob_row_bits(BJob j, const uint32_t* bits) {
    j.skip = 3;
    j.mlen = reinterpret_cast<const float*>(bits);
    return j;
}
inline BJob bjob_steps(BJob j, const float* mlen, int R, int NA, int B) {
    j.skip = 2;
    j.mlen = mlen;
    j.R = R;
    j.NA = NA;
    j.B = B;
    return j;
}

// row chunks are processed (and their partials stored) in groups of 4, one workgroup per group and output block
__host__ __device__ __forceinline__ int bjob_groups(const BJob& jb) { return (jb.chunks + 3) >> 2; }
// workgroups of a job: jobs with several output blocks take the groups in stripes of 8 (see wgrad_block_body), the
// last stripe padded with idle workgroups
__host__ __device__ __forceinline__ int bjob_stripe(const BJob& jb) { return jb.mb * jb.nb > 1 ? 8 : 1; }
__host__ __device__ __forceinline__ int bjob_wgs(const BJob& jb) {
    const int st = bjob_stripe(jb);
    return jb.mb * jb.nb * ((bjob_groups(jb) + st - 1) / st * st);
}

template <int MJ>
__device__ __forceinline__ int find_bjob(const BJobsT<MJ>& J, int task) {
    int k = 0;
    while (k + 1 < J.n && J.j[k + 1].task0 <= task) ++k;
    return k;
}

// the 8 rows rr + 8g .. rr + 8g + 7 of a lane: delta columns m0 .. m0 + 3 into a, x columns k0 .. k0 + 3 into b
// (zeros for a dead group / rows past rend / columns past M, K)
// gm: bit t = row rr + 8g + t is live
__device__ __forceinline__ void wgrad_load_step(const BJob& jb, int rr, int g, unsigned gm, int rend, int m0, int k0,
                                                bool va, bool vb, float (&a)[8][4], float (&b)[8][4]) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int row = rr + 8 * g + t;
        const bool rv = ((gm >> t) & 1u) && row < rend;
        const float* dr = jb.delta + (int64_t)row * jb.ldd + m0;
        const float* xr = jb.x + (int64_t)row * jb.ldx + k0;
        if (rv && va) {
            const floatx4 v = ld4(dr);
#pragma unroll
            for (int i = 0; i < 4; ++i) a[t][i] = v[i];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) a[t][i] = (rv && m0 + i < jb.M) ? dr[i] : 0.f;
        }
        if (rv && vb) {
            const floatx4 v = ld4(xr);
#pragma unroll
            for (int i = 0; i < 4; ++i) b[t][i] = v[i];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) b[t][i] = (rv && k0 + i < jb.K) ? xr[i] : 0.f;
        }
    }
}

// one 32-row step's products: tile i's A operand is element i of the 8 delta vectors, tile j's B operand element j
// of the 8 x vectors; x tiles split one at a time (12 VGPRs live instead of 48); every accumulator sees the same
// product sequence as with all four split up front
__device__ __forceinline__ void wgrad_mfma_step(const float (&a)[8][4], const float (&b)[8][4], floatx4 (&acc)[4][4],
                                                float (&bsum)[4]) {
    Split3 as[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        as[i] = split3(floatx4{a[0][i], a[1][i], a[2][i], a[3][i]}, floatx4{a[4][i], a[5][i], a[6][i], a[7][i]});
#pragma unroll
        for (int t = 0; t < 8; ++t) bsum[i] += a[t][i];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const Split3 bs = split3(floatx4{b[0][j], b[1][j], b[2][j], b[3][j]}, floatx4{b[4][j], b[5][j], b[6][j], b[7][j]});
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = mfma_x6(as[i], bs, acc[i][j]);
    }
}

// the work of workgroup `bid` (4 waves = 4 consecutive tasks) of a wgrad launch; a __device__ function so that
// a learner can run it as extra workgroups of another launch (learner.hip bwd4_wgrad_kernel). 256 threads.
template <int MJ, bool GLDS = false, bool REP = false>
__device__ __forceinline__ void wgrad_block_body(const BJobsT<MJ>& J, float* __restrict__ slab, int bid,
                                                 const BRepeat* rp = nullptr) {
    // partials of the 4 waves summed pairwise in LDS, (c0 + c2) + (c1 + c3), before the one slab store per workgroup
    // (two 16 KB slots: with the reverse recurrence's LDS, bwd4_wgrad_kernel still fits two workgroups per CU). GLDS:
    // 16 KB of row staging per wave, the slots in waves 2 and 3's staging (their loops are over when they fill them)
    __shared__ __attribute__((aligned(16))) floatx4 lbuf[GLDS ? 4 : 2][16][64];
    floatx4(*wred)[16][64] = GLDS ? lbuf + 2 : lbuf;
    __shared__ float wbred[2][4][16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int task = bid * 4 + w;
    const BJob& last = J.j[J.n - 1];
    // job task counts are multiples of 4: the test (and the job) is the same for the whole workgroup
    int last_rep = 1;
    if constexpr (REP) last_rep = J.n - 1 < rp->nj ? rp->rep : 1;
    if (bid * 4 >= last.task0 + bjob_wgs(last) * 4 * last_rep) return;
    const int jq = find_bjob(J, task);
    BJob jb = J.j[jq];
    int wg = (task - jb.task0) >> 2;
    if constexpr (REP) {  // repeat a of the job: a job of its own on shifted operands (workgroup-uniform)
        if (jq < rp->nj) {
            const int per = bjob_wgs(jb), a = wg / per;
            wg -= a * per;
            jb.delta += a * rp->sd[jq];
            jb.x += a * rp->sx[jq];
            jb.slab0 += (int64_t)a * jb.mb * jb.nb * bjob_groups(jb) * BSLAB;
        }
    }
    // the 4 waves of a workgroup take the row chunks 4 cg .. 4 cg + 3 of one 64 x 64 output block and add their
    // partials in LDS, so the slab holds one partial per chunk group. Jobs with several output blocks (M = 192:
    // in_trans, W_ih, W_hh; K > 64) take the groups in stripes of 8: workgroup wg of a stripe has group
    // stripe * 8 + wg % 8 and block wg / 8, so the blocks of one group are 8 workgroups apart - dispatched at about
    // the same time to the same XCD (round-robin over the 8 XCDs), where the first to read a row chunk brings it into
    // that XCD's L2 for the others
    const int nblk = jb.mb * jb.nb, st = bjob_stripe(jb);
    const int sl = wg / (st * nblk), sr = wg % (st * nblk);
    const int cg = sl * st + sr % st, blk = sr / st;
    if (cg >= bjob_groups(jb)) return;  // the last stripe's padding (whole workgroup)
    const int ch = 4 * cg + w;
    const bool act = ch < jb.chunks;  // the last group's spare waves add zeros
    const int mbi = blk / jb.nb, nbi = blk % jb.nb;
    const int col = lane & 15, g = lane >> 4;
    const int r0 = ch * jb.ch_rows, r1 = act ? min(jb.rows, r0 + jb.ch_rows) : r0;
    floatx4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = floatx4{0.f, 0.f, 0.f, 0.f};
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};
    // lane col reads the 4 consecutive delta columns m0 .. m0 + 3 and x columns k0 .. k0 + 3 of its row (one 16-byte
    // load each when the row layout allows it): MFMA tile i holds m = m0 + i, tile j holds k = k0 + j. The row (K)
    // order of every product is unchanged; only the block's output positions are permuted (undone at the store).
    const int m0 = mbi * 64 + 4 * col, k0 = nbi * 64 + 4 * col;
    const bool va = jb.va && m0 + 3 < jb.ldd, vb = jb.vb && k0 + 3 < jb.ldx;
    // 32-row steps on the bf16 matrix cores as split-bf16 fp32 emulation (six partial products, fp32 accumulation,
    // mlg_device.h mfma_x6): lane (col, g) loads rows rr + 8g .. rr + 8g + 7; K slot t of its operands = row
    // rr + 8g + t, so tile i's A operand is element i of the 8 delta vectors and tile j's B operand element j of
    // the 8 x vectors.
    // jobs that skip dead rows deal their 32-row steps to the chunks round-robin (chunk ch takes steps ch, ch +
    // chunks, ...): the live rows (a prefix of every episode) then spread evenly over the job's waves instead of
    // leaving whole chunks with all the work; other jobs keep contiguous chunks
    const bool strided = jb.skip == 1 || jb.skip == 2, rowmode = jb.skip == 3;
    const int s0 = strided ? ch : r0 >> 5, s1 = !act ? s0 : strided ? (jb.rows + 31) >> 5 : (r1 + 31) >> 5;
    const int ds = strided ? jb.chunks : 1, rend = strided ? jb.rows : r1;
    // rows with zero deltas add exactly zero: a lane's 8-row group of them loads nothing (zeros), a step with no live
    // group is skipped. The wave's steps are indexed i = 0 .. nst - 1 (step s0 + i ds); their liveness is evaluated
    // 64 steps at a time, lane l taking step index 64 win + l for the 4 row groups (four ballots), so the loop itself
    // does no integer division. With <= 64 episodes the episode lengths sit in a register (episode e in lane e).
    const int nst = act ? (s1 - s0 + ds - 1) / ds : 0;
    const int nep = jb.skip == 1 ? jb.I / jb.T : jb.B;
    const bool mreg = strided && nep <= 64;
    const float mlv = (mreg && lane < nep) ? jb.mlen[lane] : 0.f;
    int win = -1;
    uint64_t any = 0, mg = 0;  // steps of the window with a live group; this lane's group's live steps
    unsigned m32 = 0;          // rowmode: the live rows of this lane's step of the window (bit k = row k of the step)
    auto rows_live32 = [&](int row0) -> unsigned {  // the step's word of the bitmap, cut at the chunk's end
        const unsigned m = reinterpret_cast<const uint32_t*>(jb.mlen)[row0 >> 5];
        const int left = rend - row0;
        return left >= 32 ? m : (left <= 0 ? 0u : m & ((1u << left) - 1u));
    };
    auto group_live = [&](int row) -> bool {
        bool gv = row < rend;
        if (strided) {
            int eb, et;
            if (jb.skip == 1) {
                const int item = (row / jb.rpi) % jb.I;
                eb = item / jb.T;
                et = item % jb.T;
            } else {
                et = row / jb.R;
                eb = ((row % jb.R) / jb.NA) % jb.B;
            }
            const float ml = mreg ? __shfl(mlv, eb & 63) : (gv ? jb.mlen[eb] : 0.f);
            gv = gv && et < (int)ml;
        }
        return gv;
    };
    auto next_live = [&](int i) -> int {  // first step index >= i with a live group (nst: none)
        while (i < nst) {
            if ((i >> 6) != win) {
                win = i >> 6;
                const int li = (win << 6) + lane;
                const int rl = (s0 + li * ds) << 5;
                const bool inr = li < nst;
                if (rowmode) {
                    m32 = inr ? rows_live32(rl) : 0u;
                    any = __ballot(m32 != 0u);
                } else {
                    // group_live first: its lane shuffle runs with every lane active
                    const uint64_t b0 = __ballot(group_live(rl) && inr), b1 = __ballot(group_live(rl + 8) && inr),
                                   b2 = __ballot(group_live(rl + 16) && inr), b3 = __ballot(group_live(rl + 24) && inr);
                    any = b0 | b1 | b2 | b3;
                    mg = g == 0 ? b0 : g == 1 ? b1 : g == 2 ? b2 : b3;
                }
            }
            const uint64_t rem = any & (~0ull << (i & 63));
            if (rem) return (win << 6) + __builtin_ctzll(rem);
            i = (win + 1) << 6;
        }
        return nst;
    };
    // the live rows of step i (i in the current window; wave-uniform call): all 32 rows of the step in rowmode, else
    // this lane's 8-row group as a whole
    auto step_mask = [&](int i) -> unsigned {
        if (rowmode) return (unsigned)__shfl((int)m32, i & 63);
        return ((mg >> (i & 63)) & 1) ? 0xFFu << (8 * g) : 0u;
    };
    int i = next_live(0);
    unsigned gl = i < nst ? step_mask(i) : 0u;
    if constexpr (GLDS) {
        // one step ahead through LDS: the next live step's 16 row loads go global -> LDS (global_load_lds, 16 bytes
        // per lane, this wave's 16 KB of `lbuf`) while this step's products run from VGPRs (a register copy of the
        // next step does not fit in 256 VGPRs). Lanes whose rows are dead or past the end load row 0 and are zeroed
        // after the read (columns past M / K are loaded as in the register path: they only reach discarded output
        // rows / columns).
        if (__all(va && vb)) {
            floatx4(*stg)[64] = lbuf[w];
            auto issue = [&](int ii, unsigned sm) {
                const int rr = (s0 + ii * ds) << 5;
                // dead rows load a row that is there: row 0, or in rowmode the step's first live row
                const int64_t safe = (rowmode && sm) ? rr + __builtin_ctz(sm) : 0;
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const int row = rr + 8 * g + t;
                    const int64_t rs = (((sm >> (8 * g + t)) & 1u) && row < rend) ? row : safe;
                    __builtin_amdgcn_global_load_lds((const void*)(jb.delta + rs * jb.ldd + m0),
                                                     (__attribute__((address_space(3))) void*)&stg[t][0], 16, 0, 0);
                    __builtin_amdgcn_global_load_lds((const void*)(jb.x + rs * jb.ldx + k0),
                                                     (__attribute__((address_space(3))) void*)&stg[8 + t][0], 16, 0, 0);
                }
            };
            if (i < nst) issue(i, gl);
            while (i < nst) {
                const int in = next_live(i + 1);
                const unsigned gn = in < nst ? step_mask(in) : 0u;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const int rr = (s0 + i * ds) << 5;
                float a[8][4], b[8][4];
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const bool rv = ((gl >> (8 * g + t)) & 1u) && rr + 8 * g + t < rend;
                    const floatx4 va4 = stg[t][lane], vb4 = stg[8 + t][lane];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        a[t][q] = rv ? va4[q] : 0.f;
                        b[t][q] = rv ? vb4[q] : 0.f;
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the reads are done before the buffer refills
                if (in < nst) issue(in, gn);
                wgrad_mfma_step(a, b, acc, bsum);
                i = in;
                gl = gn;
            }
        }
    }
    while (i < nst) {
        float a[8][4], b[8][4];
        wgrad_load_step(jb, (s0 + i * ds) << 5, g, (gl >> (8 * g)) & 0xFFu, rend, m0, k0, va, vb, a, b);
        wgrad_mfma_step(a, b, acc, bsum);
        i = next_live(i + 1);
        gl = i < nst ? step_mask(i) : 0u;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        bsum[i] += __shfl_xor(bsum[i], 16);
        bsum[i] += __shfl_xor(bsum[i], 32);
    }
    auto put = [&](int v) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) wred[v][4 * i + j][lane] = acc[i][j];
        if (g == 0)
#pragma unroll
            for (int i = 0; i < 4; ++i) wbred[v][i][col] = bsum[i];
    };
    auto add = [&](int v) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] += wred[v][4 * i + j][lane];
            bsum[i] += wbred[v][i][col];
        }
    };
    if (w >= 2) put(w - 2);
    __syncthreads();
    if (w < 2) add(w);
    if (w == 1) put(1);  // slot 1 was read by this wave only
    __syncthreads();
    if (w != 0) return;
    add(1);
    float* out = slab + jb.slab0 + ((int64_t)blk * bjob_groups(jb) + cg) * BSLAB;
    // D layout: acc[i][j] reg q -> MFMA row 4g + q, i.e. the A values of lane col' = 4g + q (block row
    // m = 4 col' + i), and MFMA column col (block column k = 4 col + j)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *reinterpret_cast<floatx4*>(out + (4 * (4 * g + q) + i) * 64 + 4 * col) =
                floatx4{acc[i][0][q], acc[i][1][q], acc[i][2][q], acc[i][3][q]};
    if (g == 0)
#pragma unroll
        for (int i = 0; i < 4; ++i) out[4096 + 4 * col + i] = bsum[i];
}

// fixed-order sum over chunk groups -> dW / db (bias from the nbi == 0 blocks); per-block sums of squares -> nrm_part
template <int MJ>
__global__ void __launch_bounds__(256, 2) wgrad_block_kernel(BJobsT<MJ> J, float* __restrict__ slab) {
    wgrad_block_body<MJ, true>(J, slab, (int)blockIdx.x);
}

template <int MJ>
__global__ void __launch_bounds__(256, 2) wgrad_block_rep_kernel(BJobsT<MJ> J, BRepeat rp, float* __restrict__ slab) {
    wgrad_block_body<MJ, true, true>(J, slab, (int)blockIdx.x, &rp);
}

template <int MJ, bool REP = false>
__device__ __forceinline__ void wgrad_block_reduce_body(const BJobsT<MJ>& J, const float* __restrict__ slab,
                                                        float* __restrict__ nrm_part, const BRepeat* rp = nullptr) {
    __shared__ float red[256];
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t acc = 0;
    float sq = 0.f;
    for (int q = 0; q < J.n; ++q) {
        const BJob& jb = J.j[q];
        const int64_t n_one = (int64_t)jb.mb * jb.nb * BSLAB;
        int64_t n_el = n_one;
        if constexpr (REP) n_el = q < rp->nj ? n_one * rp->rep : n_one;
        if (i >= acc && i < acc + n_el) {
            int64_t loc = i - acc;
            const int ng = bjob_groups(jb);
            const float* sl = slab + jb.slab0;
            float *dw = jb.dw, *db = jb.db;
            bool dead = false;
            if constexpr (REP) {  // repeat a: its own slab range, its own dw / db
                if (q < rp->nj) {
                    const int a = (int)(loc / n_one);
                    loc -= a * n_one;
                    sl += (int64_t)a * jb.mb * jb.nb * ng * BSLAB;
                    dw += a * rp->sg;
                    if (db) db += a * rp->sg;
                    dead = rp->alive && rp->alive[a] == 0u;
                }
            }
            const int blk = (int)(loc / BSLAB), e = (int)(loc % BSLAB);
            const int mbi = blk / jb.nb, nbi = blk % jb.nb;
            float s = 0.f;
            const float* base = sl + (int64_t)blk * ng * BSLAB + e;
            int ch = 0;
            // MLG_WRED_DEPTH loads in flight (the slab partials were just written by other CUs: each round trip is an
            // L2 / MALL miss), summed in group order
            for (; ch + MLG_WRED_DEPTH <= ng; ch += MLG_WRED_DEPTH) {
                float v[MLG_WRED_DEPTH];
#pragma unroll
                for (int u = 0; u < MLG_WRED_DEPTH; ++u) v[u] = base[(int64_t)(ch + u) * BSLAB];
#pragma unroll
                for (int u = 0; u < MLG_WRED_DEPTH; ++u) s += v[u];
            }
            for (; ch + 8 <= ng; ch += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = base[(int64_t)(ch + u) * BSLAB];
#pragma unroll
                for (int u = 0; u < 8; ++u) s += v[u];
            }
            for (; ch < ng; ++ch) s += base[(int64_t)ch * BSLAB];
            if constexpr (REP) s = dead ? 0.f : s;
            if (e < 4096) {
                const int m = mbi * 64 + e / 64, k = nbi * 64 + e % 64;
                if (m < jb.M && k < jb.K) {
                    dw[(int64_t)m * jb.K + k] = s;
                    sq = s * s;
                }
            } else if (nbi == 0 && db) {
                const int m = mbi * 64 + (e - 4096);
                if (m < jb.M) {
                    db[m] = s;
                    sq = s * s;
                }
            }
            break;
        }
        acc += n_el;
    }
    const float bs = block_sum_1024(sq, red);
    if (threadIdx.x == 0) nrm_part[blockIdx.x] = bs;
}

template <int MJ>
__global__ void __launch_bounds__(256) wgrad_block_reduce_kernel(BJobsT<MJ> J, const float* __restrict__ slab,
                                                                 float* __restrict__ nrm_part) {
    wgrad_block_reduce_body<MJ>(J, slab, nrm_part);
}

template <int MJ>
__global__ void __launch_bounds__(256) wgrad_block_reduce_rep_kernel(BJobsT<MJ> J, BRepeat rp,
                                                                     const float* __restrict__ slab,
                                                                     float* __restrict__ nrm_part) {
    wgrad_block_reduce_body<MJ, true>(J, slab, nrm_part, &rp);
}

template <int MJ>
inline int64_t layout_bjobs(BJobsT<MJ>& J, int* n_tasks, int64_t* n_red, int64_t* slab_part,
                            const BRepeat* rp = nullptr) {
    int tasks = 0;
    int64_t slab = 0, red = 0;
    for (int q = 0; q < J.n; ++q) {
        const int rep = rp && q < rp->nj ? rp->rep : 1;  // a repeated job's tasks, partials and outputs, repeat-major
        J.j[q].task0 = tasks;
        J.j[q].slab0 = slab;
        tasks += bjob_wgs(J.j[q]) * 4 * rep;
        slab += (int64_t)J.j[q].mb * J.j[q].nb * bjob_groups(J.j[q]) * BSLAB * rep;
        red += (int64_t)J.j[q].mb * J.j[q].nb * BSLAB * rep;
    }
    *n_tasks = tasks;
    *n_red = red;
    *slab_part = mlg_align4(slab);
    // norm partials: one per reduce block, + 4 for a table reduced as two views (bjob_view: one more block at most)
    return mlg_align4(slab) + mlg_align4((red + 255) / 256) + 4;
}

// the wgrad launch and its fixed-order reduce over a laid-out table (host)
template <int MJ>
inline int run_jobs(const BJobsT<MJ>& J, int n_tasks, int64_t n_red, float* slab, float* nrm, hipStream_t s,
                    const char* what) {
    hipLaunchKernelGGL(wgrad_block_kernel<MJ>, dim3((unsigned)((n_tasks + 3) / 4)), dim3(256), 0, s, J, slab);
    hipLaunchKernelGGL(wgrad_block_reduce_kernel<MJ>, dim3((unsigned)((n_red + 255) / 256)), dim3(256), 0, s, J, slab,
                       nrm);
    return check_launch(what);
}

// jobs [q0, q1) of a laid-out table as a table of their own (tasks renumbered from 0, slab positions kept): the
// wgrad and reduce launches of a view compute exactly the view's dW / db (same chunks, same order), so a table can
// run as two views on two streams; the view's norm partials go to their own range of the partial array
template <int MJ>
inline BJobsT<MJ> bjob_view(const BJobsT<MJ>& J, int q0, int q1, int* n_tasks, int64_t* n_red) {
    BJobsT<MJ> V;
    V.n = 0;
    int tasks = 0;
    int64_t red = 0;
    for (int q = q0; q < q1; ++q) {
        V.j[V.n] = J.j[q];
        V.j[V.n].task0 = tasks;
        tasks += bjob_wgs(J.j[q]) * 4;
        red += (int64_t)J.j[q].mb * J.j[q].nb * BSLAB;
        ++V.n;
    }
    *n_tasks = tasks;
    *n_red = red;
    return V;
}

// clip_grad_norm_ + RMSprop for the parameter of this thread of a finish launch (1024-thread blocks over the flat
// parameter vector): every block derives the same norm from the reduce pass's per-block partials in a fixed order.
// Returns the norm. tsync: the target network copy due after this step, stored in the same launch.
__device__ __forceinline__ float clip_rmsprop_step(float* __restrict__ params, float* __restrict__ grads,
                                                   float* __restrict__ sq, int64_t n_params,
                                                   const float* __restrict__ nrm_part, int n_nrm, float lr, float alpha,
                                                   float eps, float max_norm, float* __restrict__ tsync, float* red) {
    const int tid = threadIdx.x;
    // this thread's parameter, gradient and square average, requested before the norm reduction they wait for
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + tid;
    const bool has = i < n_params;
    const float g0 = has ? grads[i] : 0.f, sq0 = has ? sq[i] : 0.f, p0 = has ? params[i] : 0.f;
    float s = 0.f;
    for (int k = tid; k < n_nrm; k += blockDim.x) s += nrm_part[k];
    const float norm = sqrtf(block_sum_1024(s, red));
    const float coef = fminf(max_norm / (norm + 1e-6f), 1.f);  // torch clip_grad_norm_ (clamped coef)
    if (has) {
        const float gi = g0 * coef;
        grads[i] = gi;
        const float a = alpha * sq0 + (1.f - alpha) * gi * gi;  // RMSprop square_avg
        sq[i] = a;
        const float pn = p0 - lr * gi / (sqrtf(a) + eps);
        params[i] = pn;
        if (tsync) tsync[i] = pn;
    }
    return norm;
}

}  // namespace mlg
