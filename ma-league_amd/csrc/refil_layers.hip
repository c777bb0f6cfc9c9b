// refil_layers.hip -- layer-level REFIL entry points (the module forward()s of the Python classes and the
// kernels the reference's layer golden vectors are checked against):
//
//   mlg_refil_attention      EntityAttentionLayer.forward over bs items (its backward: refil_grad.hip)
//                            (src/marl/modules/layers/attention.py:24-79)
//   mlg_refil_pack_mixer     FlexQMixer named_parameters -> 4 packed AttentionHyperNet blocks
//   mlg_refil_mixer_forward  FlexQMixer.forward, plain or with imagine groups (src/marl/modules/mixers/
//                            flex_qmix.py:73-117)
// Same device building blocks as the rollout / learner (refil_device.h).
#include "mlg_host.h"
#include "refil_device.h"
#include "refil_host.h"

using namespace refil;

namespace {

// ---- EntityAttentionLayer: one wave per item -------------------------------------------------------------
__global__ void __launch_bounds__(64) attention_kernel(const float* __restrict__ w_in, const float* __restrict__ w_out,
                                                       const float* __restrict__ b_out, const float* __restrict__ x,
                                                       const uint8_t* __restrict__ pre, const uint8_t* __restrict__ post,
                                                       int ne, int nq, float* __restrict__ y) {
    __shared__ float s_x[NE * LDX];
    __shared__ float s_qkv[NE * LDQ];
    __shared__ float s_o[16 * LDX];
    __shared__ uint32_t s_m[16];
    const int lane = threadIdx.x;
    const int64_t it = blockIdx.x;
    const int col = lane & 15, g = lane >> 4;
    attn_item_fwd(w_in, x + it * ne * EMB, pre + it * nq * ne, ne, nq, s_x, s_qkv, s_o, s_m, nullptr, lane);
    const bool rdead = (mask_row_bits(post + it * nq, nq) >> col) & 1u;  // post-masked rows (and those past nq)
    floatx4 yv[4];
    bias_init<4>(yv, b_out, 0, lane);
    mm_lds<4>(yv, w_out, EMB, 0, s_o, LDX, EMB / 16, lane);
    if (rdead) zero_acc<4>(yv);
    if (col < nq) {
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<floatx4*>(y + (it * nq + col) * EMB + q * 16 + 4 * g) = yv[q];
    }
}

// ---- FlexQMixer forward: one workgroup (4 waves, wave k = hypernet k) per row ----------------------------------
struct CopyJob {
    int64_t src, dst;
    int rows_dst, cols_dst, rows_src, cols_src;
};

__global__ void pack_hyper_kernel(RHyper L, const float* __restrict__ flat, float* __restrict__ packed) {
    const int k = blockIdx.y;
    const float* src = flat + (int64_t)k * L.c_total;
    float* dst = packed + (int64_t)k * L.total;
    const CopyJob J[7] = {{L.c_w1, L.w1, EMB, L.K1, EMB, L.D0},         {L.c_b1, L.b1, 1, EMB, 1, EMB},
                          {L.c_win, L.win, 3 * EMB, EMB, 3 * EMB, EMB}, {L.c_wout, L.wout, EMB, EMB, EMB, EMB},
                          {L.c_bout, L.bout, 1, EMB, 1, EMB},           {L.c_w2, L.w2, EM, EMB, EM, EMB},
                          {L.c_b2, L.b2, 1, EM, 1, EM}};
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= L.total) return;
    float v = 0.f;
    for (int q = 0; q < 7; ++q) {
        const int64_t n = (int64_t)J[q].rows_dst * J[q].cols_dst;
        if (i >= J[q].dst && i < J[q].dst + n) {
            const int64_t l = i - J[q].dst;
            const int r = (int)(l / J[q].cols_dst), c = (int)(l % J[q].cols_dst);
            if (r < J[q].rows_src && c < J[q].cols_src) v = src[J[q].src + (int64_t)r * J[q].cols_src + c];
            break;
        }
    }
    dst[i] = v;
}

struct MixFwdArgs {
    int NA, NE, D0, R, softmax;
    const float* packed;  // 4 RHyper blocks
    const float* qs;      // [R][NA or 2 NA]
    const float* ent;     // [R][NE][D0]
    const uint8_t* em;    // [R][NE]
    const uint8_t* wm;    // [R][NE][NE] or null
    const uint8_t* im;
    float* out;           // [R]
};

__global__ void __launch_bounds__(256) mixer_fwd_kernel(RHyper L, MixFwdArgs a) {
    __shared__ float s_ein[NE * LDI];
    __shared__ float s_x1[4][NE * LDX];
    __shared__ float s_qkv[4][NE * LDQ];
    __shared__ float s_o[4][16 * LDX];
    __shared__ float s_X[5][NAS * EM];  // w1 (plain or W), w1 I, w_final, b1, V
    __shared__ uint32_t s_m[4][2][16];
    const int tid = threadIdx.x, lane = tid & 63, k = tid >> 6;
    const int64_t r = blockIdx.x;
    load_entity_rows(a.ent + r * a.NE * a.D0, a.NE, a.D0, L.K1, s_ein, tid, blockDim.x);
    __syncthreads();
    // hyper_w_1 with imagine groups: W and I masks; every other hypernet: the default entity mask
    const bool two = k == 0 && a.wm != nullptr;
    const int64_t mrow = r * a.NE * a.NE;
    floatx4 x2[4], X[2];
    hyper_rows_fwd(a.packed + (int64_t)k * L.total, L, a.NA, a.NE, a.em + r * a.NE, two ? a.wm + mrow : nullptr,
                   two ? a.im + mrow : nullptr, s_ein, s_x1[k], s_qkv[k], s_o[k], s_m[k], nullptr, lane, x2, X);
    const int col = lane & 15, g = lane >> 4;
    const int v = col >> 3, n = col & 7;
    if (v < (two ? 2 : 1)) {
        const int slot = k == 0 ? v : k + 1;
#pragma unroll
        for (int q = 0; q < 2; ++q) *reinterpret_cast<floatx4*>(&s_X[slot][n * EM + q * 16 + 4 * g]) = X[q];
    }
    __syncthreads();
    if (tid >= 32) return;
    const int nrow = a.wm ? 2 * a.NA : a.NA;
    const MixRow m = mix_row(&s_X[0][0], a.qs + r * nrow, a.NA, nrow, a.softmax, tid);  // lane = embed index e
    if (tid == 0) a.out[r] = m.q_tot;
}

}  // namespace

extern "C" int mlg_refil_attention(const float* w_in, const float* w_out, const float* b_out, const float* x,
                                   const uint8_t* pre_mask, const uint8_t* post_mask, int32_t bs, int32_t ne, int32_t nq,
                                   int32_t n_heads, float* y, void* stream) {
    MLG_REQUIRE(w_in && w_out && b_out && x && pre_mask && post_mask && y, "refil_attention: null pointer");
    MLG_REQUIRE(n_heads == NH, "refil_attention: attn_n_heads=%d unsupported (4; embed 64)", n_heads);
    MLG_REQUIRE(ne >= 1 && ne <= NE && nq >= 1 && nq <= 16 && nq <= ne, "refil_attention: ne=%d nq=%d (<= 16)", ne, nq);
    if (bs <= 0) return 0;
    hipLaunchKernelGGL(attention_kernel, dim3((unsigned)bs), dim3(64), 0, (hipStream_t)stream, w_in, w_out, b_out, x,
                       pre_mask, post_mask, ne, nq, y);
    return mlg::check_launch("refil_attention");
}

int check_refil_mixer_dims(const MlgRefilDims* d) {
    MLG_REQUIRE(d != nullptr, "null refil dims");
    MLG_REQUIRE(d->n_agents >= 1 && d->n_agents <= NAS && d->n_entities >= d->n_agents && d->n_entities <= NE,
                "refil mixer: n_agents=%d n_entities=%d unsupported", d->n_agents, d->n_entities);
    MLG_REQUIRE(refil_d0(d) <= KMAX && d->attn_n_heads == NH, "refil mixer: entity input %d (<= %d), heads %d (4)",
                refil_d0(d), KMAX, d->attn_n_heads);
    return 0;
}

extern "C" int64_t mlg_refil_packed_mixer_size(const MlgRefilDims* d) {
    if (check_refil_mixer_dims(d)) return -1;
    return 4 * make_rhyper(refil_d0(d)).total;
}

extern "C" int mlg_refil_pack_mixer(const MlgRefilDims* d, const float* flat, float* packed, void* stream) {
    if (check_refil_mixer_dims(d)) return 1;
    MLG_REQUIRE(flat && packed, "refil_pack_mixer: null pointer");
    const RHyper L = make_rhyper(refil_d0(d));
    hipLaunchKernelGGL(pack_hyper_kernel, dim3((unsigned)((L.total + 255) / 256), 4), dim3(256), 0, (hipStream_t)stream, L,
                       flat, packed);
    return mlg::check_launch("refil_pack_mixer");
}

extern "C" int mlg_refil_mixer_forward(const MlgRefilDims* d, const float* packed, const float* agent_qs,
                                       const float* entities, const uint8_t* entity_mask, const uint8_t* w_mask,
                                       const uint8_t* i_mask, int32_t softmax_mixing_weights, float* q_tot, int32_t R,
                                       void* stream) {
    if (check_refil_mixer_dims(d)) return 1;
    MLG_REQUIRE(packed && agent_qs && entities && entity_mask && q_tot, "refil_mixer_forward: null pointer");
    MLG_REQUIRE((w_mask == nullptr) == (i_mask == nullptr), "refil_mixer_forward: imagine needs both W and I masks");
    if (R <= 0) return 0;
    const RHyper L = make_rhyper(refil_d0(d));
    MixFwdArgs a{d->n_agents, d->n_entities, L.D0, R, softmax_mixing_weights, packed, agent_qs, entities, entity_mask,
                 w_mask, i_mask, q_tot};
    hipLaunchKernelGGL(mixer_fwd_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, L, a);
    return mlg::check_launch("refil_mixer_forward");
}
