// refil_rollout_device.h -- device code shared by the REFIL rollouts (refil.hip: mlg_refil_rollout,
// refil_selfplay.hip: mlg_refil_rollout_selfplay): the rollout form of the entity block and of the 16-row agent
// tile, the batch slot of an env and the full-write tail zeroing. File-local in each translation unit.
#pragma once
#include "refil_device.h"

namespace refil {
namespace {

// Rollout form of entity_block (refil_device.h): the entity inputs arrive as the fc1 B operand in registers (xin,
// lane = entity row), fc1's output stays in registers as in_trans' B operand; only q (agent rows, [NAS][LDX]) and
// k | v ([NE][LDKV]) go to LDS.
constexpr int LDKV = 2 * EMB + 4;
template <int KC1>
__device__ inline void entity_block_reg(const float* __restrict__ P, const RAgent& L, const floatx4 (&xin)[KC1],
                                        float* qs, float* kvs, const uint32_t* mrow, int nq, int ne, float* o,
                                        int lane) {
    const int col = lane & 15;
    floatx4 x1[4];
    bias_init<4>(x1, P + L.b1, 0, lane);
    if constexpr (KC1 == 2) {  // K1 = 32: one split-bf16 K step over xin[0], xin[1] (wsp tiles 20-23, kk = 0)
        const u32x4* ws = reinterpret_cast<const u32x4*>(P + L.wsp) + lane;
        bf16x8 w[12];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int pc = 0; pc < 3; ++pc)
                w[mt * 3 + pc] = __builtin_bit_cast(bf16x8, ws[((REFIL_WSP_W1 + mt) * 6 + pc) * 64]);
        const Split3 xs = split3(xin[0], xin[1]);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            Split3 a;
            a.p[0] = w[mt * 3];
            a.p[1] = w[mt * 3 + 1];
            a.p[2] = w[mt * 3 + 2];
            x1[mt] = mfma_x6(a, xs, x1[mt]);
        }
    } else {
        mm_reg<4, KC1>(x1, P + L.w1, L.K1, 0, xin, lane);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) x1[i] = relu4(x1[i]);
    // in_trans as split-bf16 fp32 emulation (gru_tile_b16's scheme): x1 split once per 32-wide K step (K slot (g, i)
    // of step kk = the lane's own registers x1[2kk], x1[2kk + 1]), the weights pre-split in that K order (packed
    // section wsp), streamed in stages of 3 output tiles with the next stage's 18 loads issued before the current
    // stage's MFMAs. Tiles 0-3 = q (agent rows only), 4-11 = k | v. 144 bf16 MFMAs instead of 192 f32 MFMAs.
    {
        Split3 xs[2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) xs[kk] = split3(x1[2 * kk], x1[2 * kk + 1]);
        const u32x4* ws = reinterpret_cast<const u32x4*>(P + L.wsp) + lane;
        bf16x8 wb[2][18];  // [tile in stage * 6 + kk * 3 + piece]
        auto load = [&](int stg, bf16x8 (&w)[18]) {
#pragma unroll
            for (int i = 0; i < 18; ++i) w[i] = __builtin_bit_cast(bf16x8, ws[(stg * 18 + i) * 64]);
        };
        load(0, wb[0]);
#pragma unroll
        for (int stg = 0; stg < 4; ++stg) {
            if (stg + 1 < 4) load(stg + 1, wb[(stg + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
            const bf16x8(&w)[18] = wb[stg & 1];
#pragma unroll
            for (int ti = 0; ti < 3; ++ti) {
                const int mt = stg * 3 + ti;
                floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    Split3 a;
                    a.p[0] = w[ti * 6 + kk * 3 + 0];
                    a.p[1] = w[ti * 6 + kk * 3 + 1];
                    a.p[2] = w[ti * 6 + kk * 3 + 2];
                    acc = mfma_x6(a, xs[kk], acc);
                }
                if (mt < 4) {
                    if (col < NAS) st_row(qs, LDX, mt, acc, lane);
                } else {
                    st_row(kvs, LDKV, mt - 4, acc, lane);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    wave_sync();
    if (nq <= 8)
        attn_fwd_half(qs, LDX, kvs, kvs + EMB, LDKV, mrow, nq, ne, o, LDX, lane);
    else
        attn_fwd_split(qs, LDX, kvs, kvs + EMB, LDKV, mrow, nq, ne, o, LDX, nullptr, lane);
    wave_sync();
}

// Rollout form of agent_tile_post with out_trans and fc2 as split-bf16 fp32 emulation: o (LDS rows) is split once
// per 32-wide K step in the wsp K order (lane (col, g) reads features (2kk) * 16 + 4g .. + 3 and (2kk + 1) * 16 + 4g
// .. + 3 of row col), x2 from its D-layout registers; weights from the wsp tiles 12-19, all 48 loads issued up front.
__device__ inline void agent_tile_post_b16(const float* __restrict__ P, const RAgent& L, const float* o, uint32_t dead,
                                           floatx4 (&h)[4], int lane) {
    const int col = lane & 15, g = lane >> 4;
    const u32x4* ws = reinterpret_cast<const u32x4*>(P + L.wsp) + lane;
    bf16x8 wo[24], w2[24];  // [tile * 6 + kk * 3 + piece]
#pragma unroll
    for (int i = 0; i < 24; ++i) wo[i] = __builtin_bit_cast(bf16x8, ws[(REFIL_WSP_WOUT * 6 + i) * 64]);
    Split3 os[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
        os[kk] = split3(ld4(o + col * LDX + 2 * kk * 16 + 4 * g), ld4(o + col * LDX + (2 * kk + 1) * 16 + 4 * g));
    auto piece3 = [](const bf16x8 (&w)[24], int b) {
        Split3 s;
        s.p[0] = w[b];
        s.p[1] = w[b + 1];
        s.p[2] = w[b + 2];
        return s;
    };
    floatx4 x2[4], x3[4];
    bias_init<4>(x2, P + L.bout, 0, lane);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) x2[mt] = mfma_x6(piece3(wo, mt * 6 + kk * 3), os[kk], x2[mt]);
    // fc2's weights after out_trans' MFMAs are issued (wo's registers are free again: lower peak pressure)
#pragma unroll
    for (int i = 0; i < 24; ++i) w2[i] = __builtin_bit_cast(bf16x8, ws[(REFIL_WSP_W2 * 6 + i) * 64]);
    if ((dead >> col) & 1u) {
#pragma unroll
        for (int i = 0; i < 4; ++i) x2[i] = floatx4{0.f, 0.f, 0.f, 0.f};
    }
    Split3 xs[2];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) xs[kk] = split3(x2[2 * kk], x2[2 * kk + 1]);
    bias_init<4>(x3, P + L.b2, 0, lane);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) x3[mt] = mfma_x6(piece3(w2, mt * 6 + kk * 3), xs[kk], x3[mt]);
#pragma unroll
    for (int i = 0; i < 4; ++i) x3[i] = relu4(x3[i]);
    gru_tile_b16(P, L, x3, h, lane);
}

struct RoArgs {
    int U, NA, A, ED, S, kmin, kmax, B;
    float inv_p;
};

__device__ __forceinline__ int64_t ro_slot(const MlgEntityBatch& bt, int b) {
    return bt.ring_size > 0 ? (int64_t)((bt.ring_slot0 + b) % bt.ring_size) : (int64_t)b;
}

// zero bytes [b0, b1) of base with all 64 lanes: 16-byte stores for the aligned middle, byte stores at the edges
__device__ inline void zero_bytes(void* base, int64_t b0, int64_t b1, int lane) {
    if (b1 <= b0) return;
    uint8_t* p = reinterpret_cast<uint8_t*>(base);
    const uintptr_t ua = ((uintptr_t)(p + b0) + 15) & ~(uintptr_t)15, ub = (uintptr_t)(p + b1) & ~(uintptr_t)15;
    int64_t m0 = (int64_t)(ua - (uintptr_t)p), m1 = (int64_t)(ub - (uintptr_t)p);
    if (m0 > b1 || m1 < m0) m0 = m1 = b1;  // too short for an aligned middle
    for (int64_t i = b0 + lane; i < m0; i += 64) p[i] = 0;
    for (int64_t i = m0 + 16 * (int64_t)lane; i < m1; i += 16 * 64) *reinterpret_cast<uint4*>(p + i) = make_uint4(0, 0, 0, 0);
    for (int64_t i = (m1 > b0 ? m1 : b0) + lane; i < b1; i += 64) p[i] = 0;
}

// zero rows [t0, end) of every key of slot `slot` (full-write ring mode), all 64 lanes; end = T1, or the slot's
// extent (MlgEntityBatch.slot_extent: the rows of its previous episode that may be non-zero), which then becomes t0
__device__ inline void ro_zero_tail(const MlgEntityBatch& bt, const RoArgs& a, int64_t slot, int t0, int lane) {
    int end = bt.T1;
    if (bt.slot_extent) {
        const int x = bt.slot_extent[slot];
        end = x < 0 ? 0 : (x < bt.T1 ? x : bt.T1);
    }
    // the new extent is stored once `end` is known (the old value has been read by every lane)
    if (bt.slot_extent && lane == 0) bt.slot_extent[slot] = t0;
    if (t0 >= end) return;
    const int64_t r0 = slot * bt.T1 + t0, r1 = slot * (int64_t)bt.T1 + end;
    auto z = [&](void* p, int64_t row_bytes) { zero_bytes(p, r0 * row_bytes, r1 * row_bytes, lane); };
    z(bt.entities, (int64_t)a.U * a.ED * 4);
    z(bt.actions_onehot, (int64_t)a.NA * a.A * 4);
    z(bt.reward, 4);
    z(bt.obs_mask, (int64_t)a.U * a.U);
    z(bt.entity_mask, a.U);
    z(bt.actions, (int64_t)a.NA * 8);
    z(bt.avail, (int64_t)a.NA * a.A * 4);
    z(bt.terminated, 1);
    z(bt.filled, 8);
}

}  // namespace
}  // namespace refil
